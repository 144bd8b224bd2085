"""Stateful lifecycle tests of the flat index: a model, a schedule generator and a runner (no GPU, no import of the product).

A TRACE is plain data: {"seed", "profile", "metric", "d", "ops": [tuple, ...]}.  Every vector, id permutation, mask and query is
derived from (trace seed, the key an op carries), so a trace can be printed, pasted into a test as a literal and replayed with
run(trace, adapter).  run() applies every op to the adapter and to the MODEL and compares after every read: ids, order, counts and
distance bits (range totals and group codes too), or the error the model predicts.

THE MODEL (Model) is the append log of test_gpu_compact generalised: every row ever appended, its id, whether it is alive, plus an
int32 group code and a presence bit per id.  Its answers are oracle.flat_search over the log with the dead rows switched off
(live=), shaped by the helpers of range_data / by_id_data / distinct_data.  THE REFERENCE ADAPTER (RefIndex) keeps the same rows
but answers by another path: the survivors rebuilt as a fresh contiguous block, masked rows taken out of the block, every search
asked with its own k.  tests/test_lifecycle_cpu.py runs the pinned schedules against it, and against its MUTANTS: one stale-state
defect each, modelled on a flag of the engine; the pinned set must catch every one of them.

Store level: StoreSim states VectorStore's semantics (upsert = remove + add under the next internal id, post-filter with 3x
over-fetch, pre-filter as an id mask) over anything with the index interface: over a Model it is the store's model, over a
RefIndex the store's reference adapter.

GROUPED, RECOMMEND AND NUMERIC-FILTER READS have schedules of their own (NEW_PINNED, NEW_STORE_PINNED; _Gen9), because the
older schedules are dealt from one rng stream each and must stay op for op what they are (test_the_old_schedules_do_not_move).
  * grouped (B, k, query key, G, mask form, binding key): the model answers query b as Model.search of that query alone under
    mask group_of[b]; the reference adapter takes each group's eligible rows out of the survivors block and answers the group's
    queries in one call.  grouped_counters() predicts grouped_stats [0]-[5] from k, the live count and E_g.
  * recommend (B, k, example key, absent, mask): the model is recommend_data's fold, one search of k_b + m_b, the set strike, the
    cut; the reference adapter folds with its own loop over vector_of(id) and searches ONE depth for the batch.  recommend_stats
    [1]-[3] are compared.
  * mask kind ("numeric", leaf, const key) wherever ("compiled", code) is accepted, and the mutation numbers =
    MetaTable.set_numbers(0, first code, values): the LUT of column 0, absent at first, overwritten in crossing ranges, grown
    past its device capacity twice (Log.table_uploaded counts the regrows by vdb_meta.cpp's growth rule).
  * store level ("numeric": True in the trace): the fields ts and price, numeric filters in the pool, the reads s_recommend and
    s_with_filters, the device filter switched off and on again.

MMR, PER-GROUP AND RECOMMEND-BY-BEST READS have schedules of their own again (TWELVE_PINNED, large-twelve, TWELVE_STORE_PINNED;
_Gen12, an rng stream of its own), for the same reason.
  * mmr (B, k, query key, m, lambda key, mask): the model's candidates are Model.ranking at depth m, its picks mmr_data.select;
    query 0 of every batch lies beside the row written last.  The reference adapter searches the survivors block at depth m,
    builds the whole pair matrix and recomputes min-over-picked from it at every step.  Score bits and mmr_stats [0]-[4].
  * per_group (B, k, query key, g, mask): per_group_data.expected / routes on the full rankings and self.codes; the reference
    adapter is the host composition (its distinct answer, then one search with k = g of the eligible rows of every kept code).
    Codes, sizes, members' ids and distance bits, per_group_stats [1]-[6] under the cap set by ("set", "pg_cap", 0 | 1024).
  * best (B, k, example key, absent, mask): recommend_best_data's definition and lists_route under ("set", "rb_route", 0 | 1 | 2).
    recommend_best_data caches by case name; a life changes the rows under one name, so its PURE parts were factored out: definition()
    and lists_route() take tables=, and Model.best_tables gives them d(e, .) from Model.ranking, kept until the next mutation and
    not by name.  The reference adapter ranks the survivors block per positive, takes vector_of(id) per candidate and negative
    with oracle.distance, folds in numpy and sorts by (ordered dp, id).  dn bits and recommend_best_stats [0]-[6].
  * the op ("near", id, key, of) appends a row beside a stored one (at right angles to it, 0.01 away): as a negative it vetoes
    half of all rows, the nearest included, which no Gaussian row and no exact copy does; best_requests_of names it.
  * the generator keeps the answers it needed for its caps; pinned() hands them to slots(), so the first run() does not repeat them.
  * store level ("twelve": True): s_mmr, s_groups (a header ("#value", size) in front of every group's members), s_recommend_best."""
from collections import Counter

import numpy as np

import by_id_data as bd
import distinct_data as dd
import mmr_data as md
import oracle
import per_group_data as pgd
import range_data as rd
import recommend_best_data as rbd
import recommend_data as rcd

F32, U64, I32 = np.float32, np.uint64, np.int32
EUCLID, COSINE, DOT = 0, 1, 2
ID_LIMIT = 1 << 20                     # ids stay below: meta table and masks stay small, distinct is never refused
SMALL_N, DIRECT_MAX_Q, BF16_MIN_ROWS = 16384, 8, 65536
BATCHES, KS = (1, 8, 9, 40), (1, 10, 113, 300)
NO_DIRECT = 8                          # GpuFlatIndex.TIERS_NO_DIRECT
MUTATIONS = ("add", "bulk", "upsert", "readd", "remove", "remove_absent", "compact", "compact_shrink", "auto_compact", "codes", "reset")
READS = ("search", "masked", "sparse", "range", "by_id", "distinct")
SPARSE_SHARE = 0.02                    # eligible share of a "sparse" read's mask
# the read kinds, the mutation and the mask kind of the grouped / recommend / numeric schedules (NEW_PINNED).  The old traces never
# hold them: READS and MUTATIONS stay what the twelve + three + four old schedules were dealt from.
NEW_READS = ("grouped", "recommend", "numeric")
READS9, MUTATIONS12 = READS + NEW_READS, MUTATIONS + ("numbers",)
NUMERIC_CARRIERS = ("numeric", "masked", "by_id", "distinct", "grouped", "recommend")
# the three composed reads that came after those (TWELVE_PINNED; _Gen12): MMR, per group, recommend by best score
NEWER_READS = ("mmr", "per_group", "best")
READS12 = READS9 + NEWER_READS
MMR_MAX, BEST_MAX_K = 1024, 1024       # VDB_MMR_MAX_CANDIDATES, VDB_RECOMMEND_BEST_MAX_K
PG_LOW_CAP = 1024                      # ("set", "pg_cap", 1024): member lists above it take the giants' route
GROUP_NONE = 0xFFFFFFFF                # VDB_GROUP_NONE
GROUPED_MAX_K = 2048                   # a grouped search with k (clamped to the live count) above: one ordinary masked search per group
GROUPED_BIG_K = 2100
LEAVES = ("lt", "le", "gt", "ge", "and")   # ("numeric", leaf, const, code): Lt / Le / Gt / Ge on column 0, And([Ne(0, code), Ge(0, const)])


class Predicted(Exception):
    """an error the model (or the reference adapter) answers a read with: kind and, for VectorNotFound, the id it names"""

    def __init__(self, kind, id=None):
        super().__init__(kind, id)
        self.kind, self.id = kind, id


class Mismatch(AssertionError):
    pass


# ---------------------------------------------------------------------------------------------------------------- derived data
def rng_of(seed, key, salt=0):
    return np.random.default_rng([int(seed), int(key), int(salt)])


def vectors(seed, key, n, d, dup=0.0):
    """n gaussian rows; a share `dup` of them exact copies of other rows of the block"""
    rng = rng_of(seed, key)
    rows = rng.standard_normal((n, d)).astype(F32)
    m = int(n * dup)
    if m and n > 1:
        dst = rng.choice(n, m, replace=False)
        rows[dst] = rows[rng.integers(0, n, m)]
    return rows


def bulk_ids(seed, key, n, base, perm):
    ids = np.arange(n, dtype=np.int64)
    if perm:
        ids = rng_of(seed, key, 1).permutation(n)
    return (ids + int(base)).astype(U64)


def lists_of(gi, gd, gc):
    """(ids, dists, counts) arrays -> one (ids u64[c], distance bits u32[c]) per query"""
    return [(np.array(gi[b, :int(c)], dtype=U64), np.array(gd[b, :int(c)], dtype=F32).view(np.uint32)) for b, c in enumerate(gc)]


def k_of(ks, b):
    return int(ks) if np.isscalar(ks) else int(ks[b])


def mask_ok(mask, id_codes, present, numbers=None):
    """bool by id: ("host", ok) as it is, ("compiled", code): present and group code != code (a missing code matches, like Ne),
    ("numeric", leaf, const, code): present and numbers[code of the id] OP const -- NaN, which fails every comparison, for code
    -1, for a code at or beyond the LUT's length and for an entry set to NaN; "and": And([Ne(code), Ge(const)])"""
    if mask is None:
        return None
    if mask[0] == "host":
        return np.asarray(mask[1], dtype=bool)
    if mask[0] == "numeric":
        _, leaf, const, code = mask
        lut = np.zeros(0) if numbers is None else numbers
        has = (id_codes >= 0) & (id_codes < lut.size)
        v = np.full(id_codes.size, np.nan)
        v[has] = lut[id_codes[has]]
        with np.errstate(invalid="ignore"):
            ok = {"lt": v < const, "le": v <= const, "gt": v > const, "ge": v >= const, "and": (id_codes != I32(code)) & (v >= const)}[leaf]
        return present & ok
    return present & (id_codes != I32(mask[1]))


def on_table(mask):
    return mask is not None and mask[0] in ("compiled", "numeric")


def ok_of_ids(ok, ids):
    out = np.zeros(len(ids), dtype=bool)
    inside = ids < U64(len(ok))
    out[inside] = ok[ids[inside].astype(np.int64)]
    return out


# ---------------------------------------------------------------------------------------------------------------- the row log
class Log:
    """Every row ever appended, in order, with its id and whether it is still alive; a group code and a presence bit per id.
    Also what decides the engine's routes and re-allocations, counted from the ops alone: the capacity (1024 rows, doubling), the
    rows appended since the last read (staged), crossings of SMALL_N."""

    def __init__(self, metric, sharded=False):
        self.metric, self.sharded = int(metric), bool(sharded)
        self.rows = np.zeros((0, 0), dtype=F32)
        self.ids = np.zeros(0, dtype=U64)
        self.alive = np.zeros(0, dtype=bool)
        self.misfits = {}
        self.codes = np.full(ID_LIMIT, -1, dtype=I32)
        self.present = np.zeros(ID_LIMIT, dtype=bool)
        self.id_bound = 0
        self.cap, self.auto, self.staged, self.last_d, self.epoch = 0, 0.0, 0, 0, 0
        self.counts = dict(doublings=0, shrinks=0, up=0, down=0, dim_resets=0, auto_compactions=0, compact_with_staged=0, regrows=0)
        # the numeric LUT of column 0 by dictionary code (MetaTable.set_numbers); its device array as vdb_meta.cpp's Staged grows it:
        # at the next upload (a compile, a distinct search), to max(length, twice the old capacity, 1024) -- a REGROW when there was one
        self.numbers, self.lut_cap, self.lut_dirty, self.col_len = np.zeros(0), 0, None, 0

    # -- sizes
    @property
    def d(self):
        return self.rows.shape[1]

    def n_rows(self):
        return self.ids.size

    def n_live(self):
        return int(self.alive.sum())

    def live_ids(self):
        return np.sort(self.ids[self.alive])

    def _resized(self, before):
        n = self.n_rows()
        if before <= SMALL_N < n:
            self.counts["up"] += 1
        if n <= SMALL_N < before:
            self.counts["down"] += 1
        if n > self.cap:
            self.on_grow()
            self.cap = max(self.cap, 1024)
            while self.cap < n:
                self.cap *= 2
                self.counts["doublings"] += 1

    def on_grow(self):
        pass

    # -- mutations
    def _kill(self, ids):
        ids = np.asarray(ids, dtype=U64)
        self.epoch += 1
        self.alive &= ~np.isin(self.ids, ids)
        self.present[ids[ids < U64(ID_LIMIT)].astype(np.int64)] = False
        if self.misfits:
            for i in ids.tolist():
                self.misfits.pop(int(i), None)
        if self.ids.size and not self.alive.any():                     # the last row is gone: the store starts over
            before, self.staged = self.n_rows(), 0
            self.rows, self.ids, self.alive = np.zeros((0, 0), dtype=F32), np.zeros(0, dtype=U64), np.zeros(0, dtype=bool)
            self.cap = 0
            self.on_reset()
            self._resized(before)

    def on_reset(self):
        pass

    def add_bulk(self, rows, ids):
        self._append(rows, ids)

    def _append(self, rows, ids):
        rows, ids = np.ascontiguousarray(rows, dtype=F32), np.asarray(ids, dtype=U64)
        self._kill(ids)
        if not self.ids.size:
            if self.last_d not in (0, rows.shape[1]):
                self.counts["dim_resets"] += 1
            self.rows = np.zeros((0, rows.shape[1]), dtype=F32)
        self.last_d = rows.shape[1]
        self.epoch += 1
        before = self.n_rows()
        self.rows = np.concatenate([self.rows, self.stored(rows, before)])
        self.ids = np.concatenate([self.ids, ids])
        self.alive = np.concatenate([self.alive, np.ones(ids.size, dtype=bool)])
        self.present[ids[ids < U64(ID_LIMIT)].astype(np.int64)] = True
        self.id_bound = max(self.id_bound, int(ids.max()) + 1)
        self.staged += ids.size
        self._resized(before)

    def stored(self, rows, first):
        return rows

    def add(self, id, v):
        v = np.asarray(v, dtype=F32)
        self._kill([id])                                               # an add overwrites; the last row gone resets the store
        if self.ids.size and v.size != self.d:
            self.misfits[int(id)] = int(v.size)                        # a row of another dimension: kept aside, fails the searches
            self.id_bound = max(self.id_bound, int(id) + 1)
            return
        self._append(v[None, :], [id])

    def remove(self, ids):
        self._kill(np.atleast_1d(np.asarray(ids, dtype=U64)))

    def compact(self, shrink=False):
        """the staged rows are uploaded first, then the survivors move down; returns the rows given back"""
        if self.staged and not self.alive.all():
            self.counts["compact_with_staged"] += 1
        self.staged = 0
        self.epoch += 1
        dead = int((~self.alive).sum())
        before = self.n_rows()
        if dead:
            self.on_compact(shrink)
            self.rows, self.ids = self.rows[self.alive], self.ids[self.alive]
            self.alive = np.ones(self.ids.size, dtype=bool)
        if shrink and self.ids.size:
            cap = (self.ids.size + 1023) // 1024 * 1024
            if cap < self.cap:
                self.counts["shrinks"] += 1
            self.cap = cap
        self._resized(before)
        return dead

    def on_compact(self, shrink):
        pass

    def set_auto_compact(self, f):
        self.auto = float(f)

    def set_codes(self, first, codes):
        codes = np.asarray(codes, dtype=I32)
        self.codes[int(first):int(first) + codes.size] = codes
        self.col_len = max(self.col_len, int(first) + codes.size)

    def set_numbers(self, first, values):
        values = np.asarray(values, dtype=np.float64)
        first, end = int(first), int(first) + values.size
        if end > self.numbers.size:
            self.numbers = np.concatenate([self.numbers, np.full(end - self.numbers.size, np.nan)])
        self.numbers[first:end] = values
        lo, hi = self.lut_dirty or (first, end)
        self.lut_dirty = (min(lo, first), max(hi, end))
        self.epoch += 1

    def table_uploaded(self):
        """what a compile (and a distinct search) does to the table first: the staged LUT writes reach the device"""
        if self.numbers.size > self.lut_cap:
            if self.lut_cap:
                self.counts["regrows"] += 1
                self.on_regrow()
            self.lut_cap = max(self.numbers.size, 2 * self.lut_cap, 1024)
        self.lut_dirty = None

    def on_regrow(self):
        pass

    def numbers_seen(self):
        return self.numbers

    def ok_by_id(self, mask):
        """mask_ok over this log's columns; a mask compiled on the table uploads the table's staged writes first"""
        if on_table(mask):
            self.table_uploaded()
        return mask_ok(mask, self.codes, self.present, self.numbers_seen())

    pg_cap = rb_route = 0                  # vdb_flat_debug_set_per_group_scan_cap (0: the default), ..._recommend_best_route

    def set(self, name, value):
        if name in ("pg_cap", "rb_route"):                             # handle state: it outlives every mutation
            setattr(self, name, int(value))

    def flush(self):
        self.uploaded()

    def uploaded(self):
        """what every read and flush() does first: the staged rows reach the device, auto-compaction may run"""
        self.staged = 0
        n = self.n_rows()
        if self.auto > 0 and n and (n - self.n_live()) > self.auto * n:
            self.counts["auto_compactions"] += 1
            self.compact()

    # -- what a read answers with before it searches
    def zero_live(self):
        return self.metric == COSINE and self.ids.size and bool((self.alive & ~self.rows.any(axis=1)).any())

    def refusal(self, kind, ids=None):
        """The ORDER of the checks (include/vdb_flat.h): range, grouped and recommend by best score refuse a sharded handle before
        anything else; MMR and per group answer an empty index with empty lists BEFORE they refuse one (mmr_check,
        search_distinct_host); an absent example comes before the dimension mismatch and the zero-norm row."""
        if kind in ("range", "grouped", "best") and self.sharded:
            raise Predicted("Refused")
        if kind in ("by_id", "best"):
            live = set(self.ids[self.alive].tolist()) | set(self.misfits)
            for i in np.asarray(ids, dtype=U64).tolist():
                if i not in live:
                    raise Predicted("VectorNotFound", int(i))
        if not self.ids.size and not self.misfits:
            return True                                                # an empty store answers every query with nothing
        if kind in ("mmr", "per_group") and self.sharded:
            raise Predicted("Refused")
        if self.misfits:
            raise Predicted("DimensionMismatch")
        if self.zero_live():
            raise Predicted("InvalidVector")
        return False


# ---------------------------------------------------------------------------------------------------------------- the model
class Model(Log):
    """Expected answers from oracle.flat_search over the log with live= and nothing else.  With an index attached (driving())
    every mutation goes to the index too: the form tests/test_gpu_compact.py uses."""

    vdb = ix = None

    @classmethod
    def driving(cls, vdb, metric, rows, ix=None, **kw):
        m = cls(metric)
        m.vdb = vdb
        m.ix = ix or vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, **kw)
        m.add_bulk(rows, np.arange(rows.shape[0], dtype=U64))
        return m

    def add_bulk(self, rows, ids):
        ids = np.asarray(ids, dtype=U64)
        if self.ix is not None:
            self.ix.add_bulk(rows, ids=ids)
        super().add_bulk(rows, ids)

    def add(self, id, v):
        if self.ix is not None:
            self.ix.add(int(id), self.vdb.Vector(v))
        super().add(id, v)

    def remove(self, ids):
        if self.ix is not None:
            for i in np.atleast_1d(ids):
                self.ix.remove(int(i))
        super().remove(ids)

    def compact(self, shrink=False):
        got = self.ix.compact(shrink=shrink) if self.ix is not None else None
        dead = super().compact(shrink)
        return dead if got is None else got

    def survivors(self):
        return np.ascontiguousarray(self.rows[self.alive]), np.ascontiguousarray(self.ids[self.alive])

    def fresh(self, **kw):
        rows, ids = self.survivors()
        ix = self.vdb.GpuFlatIndex(self.vdb.DistanceMetric(self.metric), keep_host_copy=False, **kw)
        ix.add_bulk(rows, ids=ids)
        return ix

    def check(self, q, k, qsel=None, got=None, **kw):
        rows, ids = self.survivors()
        gi, gd, gc = got if got is not None else self.ix.search_batch_arrays(q, k, **kw)
        for b in (range(q.shape[0]) if qsel is None else qsel):
            oi, od = oracle.flat_search(self.metric, rows, q[b], k, ids=ids)
            assert gc[b] == len(oi), (b, gc[b], len(oi))
            assert np.array_equal(gi[b, :gc[b]], oi), (b, gi[b, :gc[b]], oi)
            assert np.array_equal(gd[b, :gc[b]].view(np.uint32), od.view(np.uint32)), (b, gd[b, :gc[b]], od)
        return gi, gd, gc

    # -- reads: the adapter interface, answered by the oracle
    def _live(self, mask):
        ok = self.ok_by_id(mask)
        live = self.alive if ok is None else self.alive & ok_of_ids(ok, self.ids)
        return live.astype(np.uint8)

    def ranking(self, q, live, k=None):
        """the oracle's ranking of one query over the log (full when k is None; the full ones are kept until the next mutation)"""
        if k is not None:
            return oracle.flat_search(self.metric, self.rows, q, k, ids=self.ids, live=live)
        memo = self.__dict__.setdefault("_memo", {})
        if memo.get("epoch") != self.epoch:
            memo.clear()
            memo["epoch"] = self.epoch
        key = (q.tobytes(), live.tobytes())
        if key not in memo:
            memo[key] = oracle.flat_search(self.metric, self.rows, q, self.n_rows(), ids=self.ids, live=live)
        return memo[key]

    def search(self, q, ks, mask=None):
        empty = self.refusal("search")
        self.uploaded()
        if empty:
            return {"lists": [(np.zeros(0, U64), np.zeros(0, np.uint32))] * len(q)}
        live = self._live(mask)
        out = []
        for b in range(len(q)):
            oi, od = self.ranking(q[b], live, k_of(ks, b))
            out.append((oi, od.view(np.uint32)))
        return {"lists": out}

    def range(self, q, radii, max_results, mask=None):
        empty = self.refusal("range")
        self.uploaded()
        if empty:
            return {"lists": [(np.zeros(0, U64), np.zeros(0, np.uint32))] * len(q), "totals": [0] * len(q)}
        live = self._live(mask)
        out, totals = [], []
        for b in range(len(q)):
            oi, od, c, total = rd.cut(self.ranking(q[b], live), radii[b], max_results)
            out.append((oi, od.view(np.uint32)))
            totals.append(total)
        return {"lists": out, "totals": totals}

    def by_id(self, ids, ks, mask=None):
        ids = np.asarray(ids, dtype=U64)
        self.refusal("by_id", ids)
        self.uploaded()
        live = self._live(mask)
        at = {int(i): r for r, i in enumerate(self.ids.tolist()) if self.alive[r]}
        sel = [at[int(i)] for i in ids]
        k = ks if np.isscalar(ks) else list(ks)
        want = bd.expected(self.metric, self.rows, sel, k, ids=self.ids, live=live)
        ans = {"lists": [(oi, od.view(np.uint32)) for oi, od, _, _ in want]}
        if np.isscalar(ks):                                          # (with per-query k the engine strikes in lists of max(k) + 1: other counts, same answers)
            ans.update(struck=sum(1 for w in want if w[2]), cut=sum(1 for w in want if w[3]))
        return ans

    def distinct(self, q, ks, mask=None):
        empty = self.refusal("distinct")
        self.uploaded()
        if empty:
            return {"lists": [(np.zeros(0, U64), np.zeros(0, np.uint32))] * len(q), "codes": [np.zeros(0, I32)] * len(q)}
        live = self._live(mask)
        out, codes, stages = [], [], []
        for b in range(len(q)):
            rank = self.ranking(q[b], live)
            ei, ed, ec = dd.expected(rank, self.codes, k_of(ks, b))
            out.append((ei, ed.view(np.uint32)))
            codes.append(ec)
            if np.isscalar(ks) and mask is None:                     # the stage that completes the query (distinct_data.stage_of)
                stages.append(dd.stage_of(rank, self.codes, int(ks), self.n_live()))
        ans = {"lists": out, "codes": codes}
        if stages:
            ans["stages"] = [stages.count(x) for x in "ABC"]
        return ans

    def grouped(self, q, ks, group_of, masks):
        """include/vdb_flat.h: "the answer for query b is what vdb_flat_search_batch returns for that query ALONE with k_b under
        mask group_of[b]".  gstats: what grouped_stats [0], [1], [2], [3], [4], [5] must read (grouped_counters)."""
        empty = self.refusal("grouped")
        self.uploaded()
        if empty:
            return {"lists": [(np.zeros(0, U64), np.zeros(0, np.uint32))] * len(q), "gstats": [len(q), 0, 0, 0, 0, 0]}
        lives = {g: self._live(masks[g]) for g in sorted({int(g) for g in group_of if g != GROUP_NONE})}
        lives[GROUP_NONE] = self._live(None)
        out = []
        for b in range(len(q)):
            oi, od = self.ranking(q[b], lives[int(group_of[b])], k_of(ks, b))
            out.append((oi, od.view(np.uint32)))
        elig = {g: int(l.sum()) for g, l in lives.items() if g != GROUP_NONE}
        return {"lists": out, "gstats": grouped_counters(ks, group_of, elig, self.n_live())}

    def recommend(self, pos, neg, ks, mask=None):
        """recommend_data.expected over the log with live=: the fold of recommend_data, the search with k_b + m_b under the mask,
        the set strike, the cut.  rstats: recommend_stats [1], [2], [3] (recommend_data.stats); cut: the requests whose list was
        longer than k_b after the strike (not an engine counter: the caps of the schedules use it)."""
        flat = np.array([i for p, n in zip(pos, neg) for i in list(p) + list(n)], dtype=U64)
        self.refusal("by_id", flat)
        self.uploaded()
        live = self._live(mask)
        at = {int(i): r for r, i in enumerate(self.ids.tolist()) if self.alive[r]}
        requests = [(tuple(at[int(i)] for i in p), tuple(at[int(i)] for i in n)) for p, n in zip(pos, neg)]
        n = len(self.rows)
        depths = [min(k_of(ks, b), n) + len(p) + len(ng) for b, (p, ng) in enumerate(requests)]
        res = oracle.search_batch(self.metric, self.rows, rcd.queries(self.rows, requests), depths, ids=self.ids, live=live)
        out, cut = [], 0
        for b, ((oi, od), (p, ng)) in enumerate(zip(res, requests)):
            keep = ~np.isin(oi, self.ids[list(p) + list(ng)])
            cut += int(keep.sum()) > k_of(ks, b)
            ei, ed = rcd.strike(oi, od, self.ids[list(p) + list(ng)], k_of(ks, b))
            out.append((ei, ed.view(np.uint32)))
        k = int(ks) if np.isscalar(ks) else [int(x) for x in ks]
        st = rcd.stats(self.metric, self.rows, requests, k, self.n_live(), ids=self.ids, live=live)
        return {"lists": out, "rstats": st[1:4], "cut": cut}

    # -- the three composed reads (NEWER_READS), each through the module that states its contract
    def row_of_live(self):
        """id -> row of the log, over the live rows"""
        at = np.nonzero(self.alive)[0]
        return dict(zip(self.ids[at].tolist(), at.tolist()))

    def mmr(self, q, ks, m, lam, mask=None):
        """include/vdb_flat.h "DIVERSE TOP-K": the candidates are the search at depth m under the mask, the picks mmr_data.select
        over their stored rows.  mstats: mmr_stats [0]-[4].  moved: the queries whose picks are not the plain top-k (a cap).  The
        schedules hold finite gaussian rows only: no pair and no score may be a NaN (the liberty of mmr_data.check is never taken)."""
        empty = self.refusal("mmr")
        self.uploaded()
        nq = len(q)
        if empty:
            return {"lists": [(np.zeros(0, U64), np.zeros(0, np.uint32))] * nq, "scores": [np.zeros(0, np.uint32)] * nq, "mstats": [nq, 0, 0, 0, 0],
                    "moved": 0}
        live, at = self._live(mask), self.row_of_live()
        out, scores, cands, pairs, moved = [], [], 0, 0, 0
        for b in range(nq):
            oi, od = self.ranking(q[b], live, min(int(m), self.n_rows()))
            vecs = self.rows[[at[int(i)] for i in oi]] if len(oi) else self.rows[:0]
            picks, sc, np_, nan = md.select(self.metric, vecs, od, k_of(ks, b), lam if np.isscalar(lam) else lam[b])
            assert not nan and not np.isnan(sc).any() and not np.isnan(od).any(), "a NaN in a lifecycle schedule"
            out.append((oi[picks], od[picks].view(np.uint32)))
            scores.append(sc.view(np.uint32))
            cands, pairs, moved = cands + len(oi), pairs + np_, moved + (list(picks) != list(range(len(picks))))
        return {"lists": out, "scores": scores, "mstats": [nq, min(int(m), self.n_live()), cands, pairs, sum(len(l[0]) for l in out)], "moved": moved}

    def per_group(self, q, ks, g, mask=None):
        """per_group_data.expected over the full rankings (kept until the next mutation, as distinct's) and self.codes.  lists: the
        representatives (what distinct answers); groups: per query [(code, member ids, member distance bits)]; pstats:
        per_group_stats [1]-[6] by per_group_data.routes under the cap currently set; deep: the largest 0-based rank of a member."""
        empty = self.refusal("per_group")
        self.uploaded()
        nq = len(q)
        if empty:
            return {"lists": [(np.zeros(0, U64), np.zeros(0, np.uint32))] * nq, "groups": [[]] * nq, "pstats": [0] * 6, "deep": -1}
        live = self._live(mask)
        ranks = [self.ranking(q[b], live) for b in range(nq)]
        out, groups, deep = [], [], -1
        for b, rank in enumerate(ranks):
            ex = pgd.expected(rank, self.codes, k_of(ks, b), g)
            groups.append([(c, ids, d.view(np.uint32)) for c, ids, d in ex])
            out.append((np.array([ids[0] for _, ids, _ in ex], dtype=U64), np.array([d[0] for _, _, d in ex], dtype=F32).view(np.uint32)))
            deep = max([deep] + [int(r[-1]) for r in pgd.member_ranks(rank, self.codes, k_of(ks, b), g)])
        k = int(ks) if np.isscalar(ks) else [int(x) for x in ks]
        return {"lists": out, "groups": groups, "pstats": pgd.routes(ranks, self.codes, k, int(g), cap=self.pg_cap or pgd.SCAN_CAP), "deep": deep}

    def best_tables(self, key, metric, rows, req, ids, elig):
        """recommend_best_data._tables without its cache by case name: d(e, .) from Model.ranking, kept until the next mutation"""
        memo = self.__dict__.setdefault("_memo", {})

        def table(e):
            oi, od = self.ranking(self.rows[e], elig)
            tkey = ("table", int(e), elig.tobytes())
            if tkey not in memo:
                at = np.nonzero(elig)[0]
                order = np.argsort(self.ids[at], kind="stable")
                t = np.full(len(rows), np.inf, dtype=F32)
                t[at[order[np.searchsorted(self.ids[at][order], oi)]]] = od
                memo[tkey] = t
            return oi, od, memo[tkey]
        return [table(e) for e in req[0]], [table(e)[2] for e in req[1]]

    def best(self, pos, neg, ks, mask=None):
        """recommend_best_data's definition (the dp fold, the strict veto, the dn fold, the order (ordered dp, id)) over the log
        with live= and the mask's rows; dn: the dn bits; bstats: recommend_best_stats [0]-[6] by lists_route on the same rankings
        under the route currently set; bstages: the stage every request ends at (not an engine output: the caps use it)."""
        flat = np.array([i for p, n in zip(pos, neg) for i in list(p) + list(n)], dtype=U64)
        self.refusal("best", flat)
        self.uploaded()
        at = self.row_of_live()
        requests = [(tuple(at[int(i)] for i in p), tuple(at[int(i)] for i in n)) for p, n in zip(pos, neg)]
        k = int(ks) if np.isscalar(ks) else [int(x) for x in ks]
        kw = dict(ids=self.ids, live=self.alive.astype(np.uint8), mask=None if mask is None else self._live(mask), tables=self.best_tables)
        want = rbd.definition(None, self.metric, self.rows, requests, k, **kw)
        routed, stages, st = rbd.lists_route(None, self.metric, self.rows, requests, k, route=self.rb_route, **kw)
        rbd.same(routed, want, "the routes restated against the definition")
        assert not any(np.isnan(d).any() or np.isnan(n).any() for _, d, n in want), "a NaN in a lifecycle schedule"
        return {"lists": [(i, d.view(np.uint32)) for i, d, _ in want], "dn": [n.view(np.uint32) for _, _, n in want], "bstats": [int(x) for x in st[:7]],
                "bstages": list(stages)}


def grouped_counters(ks, group_of, elig, n_live):
    """grouped_stats [0], [1], [2], [3], [4], [5] of one call, from k, the live count and the eligible rows E_g of every referenced
    mask (vdb_search.cpp group_plan / search_grouped).  The rule for E_g = 0: such a group is NEITHER scanned NOR sent to the
    per-group search -- its queries keep the counts 0 the output starts with and appear in no counter but [0]; so [5] sums E_g
    over the groups with 0 < E_g <= 131072 when k <= 2048, and is 0 when k > 2048 (then every group with E_g > 0 counts in [3]).
    E_g > 131072 needs more rows than these schedules hold (at most 20 000): that capacity limit is out of their reach."""
    kmax = int(ks) if np.isscalar(ks) else max(int(x) for x in ks)
    scan = min(kmax, max(n_live, 1)) <= GROUPED_MAX_K
    some = [int(g) for g in group_of if g != GROUP_NONE and elig[int(g)] > 0]
    return [len(group_of), len(elig), len(some) if scan else 0, 0 if scan else len(some), sum(1 for g in group_of if g == GROUP_NONE),
            sum(elig[g] for g in set(some)) if scan else 0]


# ---------------------------------------------------------------------------------------------------------------- the reference adapter
class RefIndex(Log):
    """The same rows, answered by another path: the survivors as a fresh contiguous block (Model.fresh() without a GPU), masked
    rows removed from the block instead of switched off, every search asked with its own k."""

    def seen(self):
        """(rows, ids, alive) as the reads see them: the hook of most mutants"""
        return self.rows, self.ids, self.alive

    def block(self, mask):
        rows, ids, alive = self.seen()
        keep = alive.copy()
        ok = self.ok_by_id(mask)
        if ok is not None:
            keep &= ok_of_ids(ok, ids)
        return np.ascontiguousarray(rows[keep]), np.ascontiguousarray(ids[keep])

    def knn(self, rows, ids, q, k):
        return oracle.flat_search(self.metric, rows, q, k, ids=ids)

    def search(self, q, ks, mask=None):
        empty = self.refusal("search")
        self.uploaded()
        rows, ids = self.block(mask)
        if empty:
            rows = np.zeros((0, q.shape[1]), dtype=F32)
        out = []
        for b in range(len(q)):
            oi, od = self.knn(rows, ids, q[b], k_of(ks, b)) if len(rows) else (np.zeros(0, U64), np.zeros(0, F32))
            out.append((oi, od.view(np.uint32)))
        return {"lists": out}

    def range_total(self, q, r, mask, total):
        return total

    def range(self, q, radii, max_results, mask=None):
        empty = self.refusal("range")
        self.uploaded()
        rows, ids = self.block(mask)
        out, totals = [], []
        for b in range(len(q)):
            if empty or not len(rows):
                out.append((np.zeros(0, U64), np.zeros(0, np.uint32)))
                totals.append(0)
                continue
            oi, od, c, total = rd.cut(self.knn(rows, ids, q[b], len(rows)), radii[b], max_results)
            out.append((oi, od.view(np.uint32)))
            totals.append(self.range_total(q[b], radii[b], mask, total))
        return {"lists": out, "totals": totals}

    def vector_of(self, id):
        rows, ids, alive = self.seen()
        at = np.nonzero(alive & (ids == U64(id)))[0]
        if not at.size:
            raise Predicted("VectorNotFound", int(id))
        return rows[at[-1]]

    def by_id(self, ids, ks, mask=None):
        ids = np.asarray(ids, dtype=U64)
        self.refusal("by_id", ids)
        self.uploaded()
        rows, bids = self.block(mask)
        out, struck, cut = [], 0, 0
        for b, own in enumerate(ids):
            k = k_of(ks, b)
            oi, od = self.knn(rows, bids, self.vector_of(own), k + 1) if len(rows) else (np.zeros(0, U64), np.zeros(0, F32))
            oi, od, hit, _cut = bd.strike(oi, od, own, k)
            struck += bool(hit)
            cut += bool(_cut)
            out.append((oi, od.view(np.uint32)))
        return {"lists": out, "struck": struck, "cut": cut} if np.isscalar(ks) else {"lists": out}

    def codes_seen(self):
        return self.codes

    def distinct(self, q, ks, mask=None):
        empty = self.refusal("distinct")
        self.uploaded()
        rows, ids = self.block(mask)
        out, codes = [], []
        for b in range(len(q)):
            if empty or not len(rows):
                out.append((np.zeros(0, U64), np.zeros(0, np.uint32)))
                codes.append(np.zeros(0, I32))
                continue
            ei, ed, ec = dd.expected(self.knn(rows, ids, q[b], len(rows)), self.codes_seen(), k_of(ks, b))
            out.append((ei, ed.view(np.uint32)))
            codes.append(ec)
        return {"lists": out, "codes": codes}

    # -- grouped: per group, the group's eligible rows taken out of the survivors block, all its queries in one knn_batch call
    def knn_batch(self, rows, ids, q, ks):
        return oracle.search_batch(self.metric, rows, q, ks, ids=ids)

    def view_before_upload(self):
        """(rows, ids, alive) as the unfiltered queries and the k > 2048 fallback of a grouped read see them, taken BEFORE the
        read uploads the staged rows; None: as every other query sees them (hook of GroupedSideSkipsFlush)"""
        return None

    def group_keeps(self, masks, refs, view):
        """bool by row of `view` for every referenced mask: alive and eligible (hook of the grouped mutants)"""
        rows, ids, alive = view
        return [alive & ok_of_ids(self.ok_by_id(masks[g]), ids) for g in refs]

    def grouped(self, q, ks, group_of, masks):
        empty = self.refusal("grouped")
        early = self.view_before_upload()
        self.uploaded()
        nq = len(q)
        out = [(np.zeros(0, U64), np.zeros(0, np.uint32))] * nq
        if empty:
            return {"lists": out, "gstats": [nq, 0, 0, 0, 0, 0]}
        view = self.seen()
        refs = sorted({int(g) for g in group_of if g != GROUP_NONE})
        keeps = dict(zip(refs, self.group_keeps(masks, refs, view)))
        kmax = int(ks) if np.isscalar(ks) else max(int(x) for x in ks)
        fallback = min(kmax, max(self.n_live(), 1)) > GROUPED_MAX_K
        for g in refs + [GROUP_NONE]:
            members = [b for b in range(nq) if int(group_of[b]) == g]
            side = early is not None and (g == GROUP_NONE or fallback)
            rows, ids, alive = early if side else view
            if g == GROUP_NONE:
                keep = alive
            elif side:
                keep = alive & ok_of_ids(self.ok_by_id(masks[g]), ids)
            else:
                keep = keeps[g]
            if not members or not keep.any():
                continue
            block, bids = np.ascontiguousarray(rows[keep]), np.ascontiguousarray(ids[keep])
            for b, (oi, od) in zip(members, self.knn_batch(block, bids, q[members], [k_of(ks, b) for b in members])):
                out[b] = (oi, od.view(np.uint32))
        elig = {g: int(keeps[g].sum()) for g in refs}
        return {"lists": out, "gstats": grouped_counters(ks, group_of, elig, self.n_live())}

    # -- recommend: its own fold over vector_of(id), f32, left to right, one multiply by F32(1) / F32(n); the survivors block
    def average(self, ids, first=0):
        with np.errstate(over="ignore", invalid="ignore"):
            s = self.example_of(ids[0], first).astype(F32, copy=True)
            for j, i in enumerate(ids[1:]):
                s = s + self.example_of(i, first + 1 + j)
            return s if len(ids) == 1 else s * (F32(1) / F32(len(ids)))

    def example_of(self, id, position):
        """the stored vector of an example; position: its place in the request (positives first)"""
        return self.vector_of(id)

    def resolve_before_upload(self, flat):
        pass

    def struck_ids(self, pos, neg):
        return np.array(list(pos) + list(neg), dtype=U64)

    def recommend(self, pos, neg, ks, mask=None):
        flat = np.array([i for p, n in zip(pos, neg) for i in list(p) + list(n)], dtype=U64)
        self.refusal("by_id", flat)
        self.resolve_before_upload(flat)
        self.uploaded()
        rows, bids = self.block(mask)
        out, struck_total = [], 0
        kmax = int(ks) if np.isscalar(ks) else max(int(x) for x in ks)
        kcut = min(kmax, max(self.n_live(), 1))
        mmax = max(len(p) + len(n) for p, n in zip(pos, neg))
        for b, (p, n) in enumerate(zip(pos, neg)):
            ap = self.average(list(p))
            with np.errstate(over="ignore", invalid="ignore"):
                fold = ap if not len(n) else ap + (ap - self.average(list(n), len(p)))
            k, m = k_of(ks, b), len(p) + len(n)
            oi, od = self.knn(rows, bids, fold, kcut + mmax) if len(rows) else (np.zeros(0, U64), np.zeros(0, F32))
            oi, od = oi[:min(kcut + mmax, self.n_live())], od[:min(kcut + mmax, self.n_live())]
            hit = np.isin(oi, self.struck_ids(p, n))
            struck_total += int((hit & (np.cumsum(~hit) - ~hit < kcut)).sum())      # (the examples in front of the cut of the batch-wide list)
            out.append((oi[~hit][:k], od[~hit][:k].view(np.uint32)))
        return {"lists": out, "rstats": [len(flat), struck_total, min(kcut + mmax, self.n_live())]}

    # -- MMR: its own depth-m search of the survivors block, the whole c x c pair matrix, and the greedy choice with min over
    # the picked recomputed from the matrix at every step (the naive form, not select()'s incremental near)
    def mmr_vectors(self, ids):
        """the stored rows the candidate ids resolve to (hook of the MMR mutants)"""
        return np.stack([self.vector_of(i) for i in ids])

    def pair_matrix(self, vecs):
        """D(i, j) for all i, j by oracle.distance; above 32 candidates (1024 x 1024 calls take 9 s) row i is one oracle search of
        the candidate block with candidate i as the query, scattered back by position -- the same arithmetic"""
        c = len(vecs)
        D = np.zeros((c, c), dtype=F32)
        if c <= 32:
            for i in range(c):
                for j in range(c):
                    D[i, j] = md.pair_distance(self.metric, vecs[i], vecs[j])
            return D
        block = np.ascontiguousarray(vecs, dtype=F32)
        for i in range(c):
            oi, od = oracle.flat_search(self.metric, block, block[i], c)
            D[i, oi.astype(np.int64)] = od
        return D

    def mmr(self, q, ks, m, lam, mask=None):
        empty = self.refusal("mmr")
        self.uploaded()
        nq = len(q)
        rows, ids = self.block(mask)
        out, scores, cands, pairs = [], [], 0, 0
        for b in range(nq):
            if empty or not len(rows):
                out.append((np.zeros(0, U64), np.zeros(0, np.uint32)))
                scores.append(np.zeros(0, np.uint32))
                continue
            oi, od = self.knn(rows, ids, q[b], min(int(m), len(rows)))
            c, count = len(oi), min(k_of(ks, b), len(oi))
            l = F32(lam if np.isscalar(lam) else lam[b])
            mu = F32(1) - l
            D = self.pair_matrix(self.mmr_vectors(oi)) if count > 1 else None
            picks, sc = [0], [F32(l * od[0])]
            for t in range(1, count):
                rest = np.array([i for i in range(c) if i not in picks])
                near = D[np.ix_(rest, picks)].min(axis=1)
                score = (l * od[rest]).astype(F32) - (mu * near).astype(F32)
                j = int(np.argmin(score))                            # (the first of equal scores: the lower position)
                picks.append(int(rest[j]))
                sc.append(score[j])
                pairs += len(rest)
            out.append((oi[picks], od[picks].view(np.uint32)))
            scores.append(np.asarray(sc, dtype=F32).view(np.uint32))
            cands += c
        depth = 0 if empty else min(int(m), self.n_live())
        return {"lists": out, "scores": scores, "mstats": [nq, depth, cands, pairs, sum(len(l_[0]) for l_ in out)]}

    # -- per group: the host composition -- its own distinct answer, then for every kept code c >= 0 one search with k = g of
    # the survivors block cut down to the eligible rows with that code
    def listing_codes(self):
        """the code column as the member listing reads it (hook)"""
        return self.codes_seen()

    def listing_block(self, mask):
        """(rows, ids) the member listing walks (hook)"""
        return self.block(mask)

    def giant_block(self, mask):
        """(rows, ids) the masked search of a giant code runs over (hook)"""
        return self.block(mask)

    def per_group(self, q, ks, g, mask=None):
        empty = self.refusal("per_group")
        self.uploaded()
        nq, g = len(q), int(g)
        if empty:
            return {"lists": [(np.zeros(0, U64), np.zeros(0, np.uint32))] * nq, "groups": [[]] * nq, "pstats": [0] * 6}
        rows, ids = self.block(mask)
        lrows, lids = self.listing_block(mask)
        lcodes = dd.codes_of(lids, self.listing_codes())
        cap = self.pg_cap or pgd.SCAN_CAP
        out, groups, size, st = [], [], {}, dict(groups=0, filled=0, giant=0, evaluated=0)
        for b in range(nq):
            if not len(rows):
                out.append((np.zeros(0, U64), np.zeros(0, np.uint32)))
                groups.append([])
                continue
            ei, ed, ec = dd.expected(self.knn(rows, ids, q[b], len(rows)), self.codes_seen(), k_of(ks, b))
            mine = []
            for i, d, c in zip(ei, ed, ec):
                if c < 0 or g == 1:
                    mine.append((int(c), np.array([i], dtype=U64), np.array([d], dtype=F32).view(np.uint32)))
                    if c >= 0:
                        size[int(c)] = 0
                    continue
                e = size[int(c)] = int((lcodes == c).sum())
                if e <= cap:
                    sel, (brows, bids) = lcodes == c, (lrows, lids)
                    st["filled"], st["evaluated"] = st["filled"] + 1, st["evaluated"] + e
                else:
                    brows, bids = self.giant_block(mask)
                    sel = dd.codes_of(bids, self.listing_codes()) == c
                    st["giant"] += 1
                mi, md_ = self.knn(np.ascontiguousarray(brows[sel]), np.ascontiguousarray(bids[sel]), q[b], g) if sel.any() else (np.zeros(0, U64), np.zeros(0, F32))
                mine.append((int(c), mi, md_.view(np.uint32)))
            st["groups"] += len(mine)
            groups.append(mine)
            out.append((ei, ed.view(np.uint32)))
        listed = 0 if g == 1 else sum(e for e in size.values() if e <= cap)
        return {"lists": out, "groups": groups, "pstats": [st["groups"], st["filled"], st["giant"], len(size), listed, st["evaluated"]]}

    # -- recommend by best score: the host composition -- one full-depth ranking of the survivors block per positive (by id: the
    # query is vector_of), vector_of(id) per candidate and per negative with oracle.distance, the folds in numpy, the order
    # (ordered dp, id).  The stages (for bstats) from the same rankings cut at the stage depths, by a walk of its own (candidates_at).
    def veto_vector(self, id):
        """the stored row a candidate id resolves to in the veto (hook)"""
        return self.vector_of(id)

    def stage_block(self, stage, mask):
        """(rows, ids) the lists of stage 0 / 1 are searched over, and those the exact scan (stage 2) walks (hook)"""
        return self.block(mask)

    def route_seen(self):
        return self.rb_route

    WALK_ROWS, WALK_ENTRIES = 1024, 4096                             # the rows a request walks, the entries it merges

    def candidates_at(self, lists, D, examples):
        """The candidates of one request from its positives' lists cut at depth D, in the words of include/vdb_flat.h and
        DESIGN.md 4.17 and in numpy (the model goes through recommend_best_data._walk, a loop over tuples): a list with D
        entries ends at its frontier, F is the smallest frontier, an entry with d < F is settled; beyond WALK_ENTRIES settled
        entries only those in front of the first entry past the capacity count; per id the smallest distance; the examples
        struck; ascending by (dp, -0.0 in front of +0.0, id), WALK_ROWS rows at most.  Returns (ids, open): open when something
        may lie behind the candidates -- a list that came back full, the capacity, the row limit."""
        cut = [(oi[:D], od[:D]) for oi, od in lists]
        fronts = [od[-1] for _, od in cut if len(od) == D]
        is_open = bool(fronts)
        ids = np.concatenate([oi for oi, _ in cut]) if cut else np.zeros(0, U64)
        d = np.concatenate([od for _, od in cut]) if cut else np.zeros(0, F32)
        which = np.concatenate([np.full(len(oi), i) for i, (oi, _) in enumerate(cut)]) if cut else np.zeros(0, int)
        if fronts:
            settled = d < min(fronts)
            ids, d, which = ids[settled], d[settled], which[settled]
        if len(d) > self.WALK_ENTRIES:
            order = np.lexsort((which, ids, ~np.signbit(d), d))
            at = order[self.WALK_ENTRIES]
            front = (d < d[at]) | ((d == d[at]) & np.signbit(d) & ~np.signbit(d[at]))
            ids, d, which, is_open = ids[front], d[front], which[front], True
        first = np.lexsort((which, d, ids))                          # per id its smallest distance (of equal ones the earlier list's bits)
        keep = first[np.concatenate([[True], ids[first][1:] != ids[first][:-1]])] if len(first) else first
        ids, d = ids[keep], d[keep]
        mine = ~np.isin(ids, np.array(sorted(examples), dtype=U64))
        ids, d = ids[mine], d[mine]
        order = np.lexsort((ids, ~np.signbit(d), d))
        if len(order) > self.WALK_ROWS:
            order, is_open = order[:self.WALK_ROWS], True
        return ids[order].tolist(), is_open

    def best(self, pos, neg, ks, mask=None):
        flat = np.array([i for p, n in zip(pos, neg) for i in list(p) + list(n)], dtype=U64)
        self.refusal("best", flat)
        self.resolve_before_upload(flat)
        self.uploaded()
        nl = self.n_live()
        kmax = int(ks) if np.isscalar(ks) else max(int(x) for x in ks)
        kcut, mmax = min(kmax, nl), max(len(p) + len(n) for p, n in zip(pos, neg))
        D0, D1 = min(nl, 1024, max(2 * (min(kcut, 1024) + min(mmax, 1024)), 32)), min(nl, 1024)   # (include/vdb_flat.h: the stage depths)
        route = self.route_seen()
        use_lists = route == rbd.LISTS or (route == rbd.AUTO and D0 < nl)
        depths = ([D0] + ([D1] if D1 > D0 else [])) if use_lists else []
        out, dns, stages, searches = [], [], [], 0
        for b, (p, n) in enumerate(zip(pos, neg)):
            kb = min(k_of(ks, b), kcut)
            examples = {int(i) for i in list(p) + list(n)}
            pvecs = [self.example_of(i, j) for j, i in enumerate(p)]
            nvecs = [self.example_of(i, len(p) + j) for j, i in enumerate(n)]

            def kept_of(cands, dp_of):
                """walk (id, dp) candidates in order: the veto with oracle.distance per candidate and negative, until kb are kept"""
                good = []
                for x in cands:
                    if len(good) == kb:
                        break
                    if not nvecs:
                        good.append((x, dp_of[x], F32(np.inf)))
                        continue
                    v, dn = self.veto_vector(x), F32(np.inf)
                    veto = False
                    for j, nv in enumerate(nvecs):
                        t = md.pair_distance(self.metric, nv, v)
                        veto = veto or not dp_of[x] < t
                        dn = t if j == 0 or t < dn else dn
                    if not veto:
                        good.append((x, dp_of[x], dn))
                return good

            def folded(rows, bids):
                """dp per id of a block: a left fold of the positives' full rankings, and the ids by (ordered dp, id)"""
                order = np.argsort(bids, kind="stable")
                dp = None
                lists = []
                for v in pvecs:
                    oi, od = self.knn(rows, bids, v, len(rows)) if len(rows) else (np.zeros(0, U64), np.zeros(0, F32))
                    lists.append((oi, od))
                    t = np.zeros(len(bids), dtype=F32)
                    t[order[np.searchsorted(bids[order], oi)]] = od
                    dp = t if dp is None else np.where(t < dp, t, dp)
                return lists, dp

            done = None
            for stage, D in enumerate(depths):
                searches += len(p)
                rows, bids = self.stage_block(stage, mask)
                lists, dp = folded(rows, bids)
                walk, is_open = self.candidates_at(lists, D, examples)
                dp_of = dict(zip(bids.tolist(), dp))
                good = kept_of(walk, dp_of)
                if len(good) >= kb or not is_open:
                    done = (stage, good)
                    break
            if done is None:
                rows, bids = self.stage_block(rbd.STAGE_SCAN, mask)
                _, dp = folded(rows, bids)
                cand = ~np.isin(bids, np.array(sorted(examples), dtype=U64))
                o = np.lexsort((bids[cand], ~np.signbit(dp[cand]), dp[cand]))          # (dp ascending, -0.0 in front of +0.0, then the id)
                done = (rbd.STAGE_SCAN, kept_of(bids[cand][o].tolist(), dict(zip(bids.tolist(), dp))))
            stages.append(done[0])
            good = done[1][:kb]
            out.append((np.array([x for x, _, _ in good], dtype=U64), np.array([d for _, d, _ in good], dtype=F32).view(np.uint32)))
            dns.append(np.array([t for _, _, t in good], dtype=F32).view(np.uint32))
        st = [len(pos), len(flat), stages.count(0), stages.count(1), stages.count(rbd.STAGE_SCAN), D0, searches]
        return {"lists": out, "dn": dns, "bstats": st}


# ---------------------------------------------------------------------------------------------------------------- mutants
class LostRemove(RefIndex):
    """1. a remove is not seen by reads until the next add (live_dirty lost)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.unseen = np.zeros(0, dtype=bool)

    def remove(self, ids):
        before = self.alive.copy()
        super().remove(ids)
        if self.alive.size == before.size:
            u = np.zeros(before.size, dtype=bool)
            u[:self.unseen.size] = self.unseen[:before.size]
            self.unseen = u | (before & ~self.alive)

    def _append(self, rows, ids):
        self.unseen = np.zeros(0, dtype=bool)
        super()._append(rows, ids)

    def on_compact(self, shrink):
        self.unseen = np.zeros(0, dtype=bool)

    def seen(self):
        alive = self.alive.copy()
        n = min(alive.size, self.unseen.size)
        alive[:n] |= self.unseen[:n]
        return self.rows, self.ids, alive


class StagedInvisibleOnce(RefIndex):
    """2. rows staged since the last read are invisible to the NEXT read only (n_uploaded / pending)"""

    def seen(self):
        alive = self.alive.copy()
        if self.staged:
            alive[self.n_rows() - self.staged:] = False
        return self.rows, self.ids, alive

    def search(self, *a, **kw):
        return self._late(super().search, *a, **kw)

    def range(self, *a, **kw):
        return self._late(super().range, *a, **kw)

    def by_id(self, *a, **kw):
        return self._late(super().by_id, *a, **kw)

    def distinct(self, *a, **kw):
        return self._late(super().distinct, *a, **kw)

    def uploaded(self):
        pass

    def flush(self):
        Log.uploaded(self)

    def _late(self, read, *a, **kw):
        try:
            return read(*a, **kw)
        finally:
            Log.uploaded(self)


class IdsNotMoved(RefIndex):
    """3. after a compaction the id column is not moved with the rows beyond the first dead one"""

    def on_compact(self, shrink):
        self._old_ids = self.ids.copy()

    def compact(self, shrink=False):
        self._old_ids = None
        dead = super().compact(shrink)
        if self._old_ids is not None:
            self.ids = self._old_ids[:self.ids.size].copy()
        return dead


class GrowForgetsTombstones(RefIndex):
    """4. a capacity doubling forgets the tombstones of old rows"""

    def on_grow(self):
        if self.cap:
            self._revive = True

    def _append(self, rows, ids):
        self._revive = False
        n = self.n_rows()
        super()._append(rows, ids)
        if self._revive and self.n_rows() > n:
            self.alive[:n] = True


class SampleKeyCollision(RefIndex):
    """5. shrink-compaction followed by adds back to the same row count serves the row block from before: a copy of the rows
    keyed only by the row count (sample16_n), which an ordinary compaction drops and a shrinking one forgets to"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.copy = {}

    def on_compact(self, shrink):
        if not shrink:
            self.copy = {}

    def on_reset(self):
        self.copy = {}

    def seen(self):
        n = self.n_rows()
        held = self.copy.get(n)
        if held is None or held.shape != self.rows.shape:
            held = self.copy[n] = self.rows.copy()
        return held, self.ids, self.alive


class TiesByPosition(RefIndex):
    """6. ties are broken by row position instead of id once ids are non-monotone (rank_valid)"""

    def knn(self, rows, ids, q, k):
        oi, od = oracle.flat_search(self.metric, rows, q, k)
        return ids[oi.astype(np.int64)], od


class StaleZeroFlag(RefIndex):
    """7. a removed zero-norm row still fails Cosine searches, and an added one does not yet (zero_valid): the flag a read uses
    is the one the read before it computed"""

    flag = False

    def zero_live(self):
        now, was = super().zero_live(), self.flag
        self.flag = now
        return was

    def block(self, mask):
        rows, ids = super().block(mask)
        keep = rows.any(axis=1) if self.metric == COSINE and len(rows) else np.ones(len(rows), dtype=bool)
        return np.ascontiguousarray(rows[keep]), np.ascontiguousarray(ids[keep])


class ByIdGathersOldRow(RefIndex):
    """8. search by id gathers the row the id had before its upsert"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.before = {}

    def _append(self, rows, ids):
        live = {int(i): r for r, i in enumerate(self.ids.tolist()) if self.alive[r]}
        for j, i in enumerate(np.asarray(ids, dtype=U64).tolist()):
            if i in live and self.rows.shape[1] == np.shape(rows)[1]:
                self.before[i] = self.rows[live[i]].copy()
        super()._append(rows, ids)

    def add(self, id, v):
        at = np.nonzero(self.alive & (self.ids == U64(id)))[0]
        if at.size and self.d == np.size(v):
            self.before[int(id)] = self.rows[at[-1]].copy()
        super().add(id, v)

    def on_reset(self):
        self.before = {}

    def vector_of(self, id):
        v = super().vector_of(id)
        return self.before.get(int(id), v)


class TotalCountsDead(RefIndex):
    """9. the range total counts dead rows"""

    def range_total(self, q, r, mask, total):
        rows, ids, alive = self.seen()
        dead = np.ascontiguousarray(rows[~alive])
        if not len(dead):
            return total
        _, od = oracle.flat_search(self.metric, dead, q, len(dead))
        with np.errstate(invalid="ignore"):
            return total + int((od <= F32(r)).sum())


class CodesLostAfterDistinct(RefIndex):
    """10. a group-code write made after a distinct search never reaches the column (Staged range lost)"""

    column = None

    def distinct(self, *a, **kw):
        out = super().distinct(*a, **kw)
        if self.column is None:
            self.column = self.codes.copy()
        return out

    def codes_seen(self):
        return self.codes if self.column is None else self.column


class RefillKeepsNorms(RefIndex):
    """12. remove-everything-then-refill keeps the per-row norms of the old rows"""

    old = np.zeros(0)

    def _kill(self, ids):
        norms = np.sqrt((self.rows.astype(np.float64) ** 2).sum(axis=1)) if self.ids.size else None
        super()._kill(ids)
        if norms is not None and not self.ids.size:
            self.old = norms

    def stored(self, rows, first):
        n = max(0, min(len(rows), self.old.size - first))
        if not n:
            return rows
        rows = rows.copy()
        now = np.sqrt((rows[:n].astype(np.float64) ** 2).sum(axis=1))
        scale = np.where(now > 0, self.old[first:first + n] / np.where(now > 0, now, 1.0), 1.0)
        rows[:n] = (rows[:n] * scale[:, None]).astype(F32)
        return rows


class GroupedIgnoresLive(RefIndex):
    """13. grouped: the row mask is mask_g[row_ids] alone, without the live bit -- a removed row stays eligible until a compaction"""

    def group_keeps(self, masks, refs, view):
        rows, ids, alive = view
        return [ok_of_ids(self.ok_by_id(masks[g]), ids) for g in refs]


class GroupedSideSkipsFlush(RefIndex):
    """14. grouped: the unfiltered queries and the k > 2048 fallback skip the flush -- rows staged since the last read are
    invisible to those queries only"""

    def view_before_upload(self):
        rows, ids, alive = self.seen()
        alive = alive.copy()
        if self.staged:
            alive[self.n_rows() - self.staged:] = False
        return rows, ids, alive


class GroupedKeepsRowMasks(RefIndex):
    """15. grouped: the row masks of the previous grouped read are kept when the row count and the number of referenced masks
    are unchanged (a workspace keyed by its sizes, like 5)"""

    held = None

    def group_keeps(self, masks, refs, view):
        key = (len(view[1]), len(refs))
        if self.held is None or self.held[0] != key:
            self.held = (key, super().group_keeps(masks, refs, view))
        return self.held[1]


class RecommendResolvesEarly(RefIndex):
    """16. recommend: the examples' row numbers are resolved before the compaction the same read triggers -- the fold takes
    whatever sits at the old row numbers"""

    def resolve_before_upload(self, flat):
        self.early = {int(i): r for r, i in enumerate(self.ids.tolist()) if self.alive[r]}

    def example_of(self, id, position):
        return self.rows[min(self.early[int(id)], self.n_rows() - 1)]


class RecommendFoldsOldRow(ByIdGathersOldRow):
    """17. recommend: every example but the first of a request is the row its id had before the upsert (8 does not see this:
    search by id is right, and so is the request ([x], []))"""

    def vector_of(self, id):
        return RefIndex.vector_of(self, id)

    def example_of(self, id, position):
        v = RefIndex.vector_of(self, id)
        return self.before.get(int(id), v) if position else v


class RecommendStrikesOnce(RefIndex):
    """18. recommend: the strike goes by the position of an id's first listing, and a second listing of the same id takes the
    strike back -- an id listed twice is returned as a neighbour"""

    def struck_ids(self, pos, neg):
        listed = Counter(int(i) for i in list(pos) + list(neg))
        return np.array([i for i, c in listed.items() if c == 1], dtype=U64)


class RegrowDropsLut(RefIndex):
    """19. a regrow of the LUT's device array drops the entries the device had: they read NaN until they are set again"""

    def on_regrow(self):
        lo, hi = self.lut_dirty or (0, 0)
        kept = self.numbers[lo:hi].copy()
        self.numbers[:] = np.nan
        self.numbers[lo:hi] = kept


class LutDirtyLastCall(RefIndex):
    """20. the LUT's dirty range covers only the last set_numbers call before a compile: an earlier, disjoint call is lost
    (until a regrow sends the whole array)"""

    dev, last = np.zeros(0), None

    def set_numbers(self, first, values):
        super().set_numbers(first, values)
        self.last = (int(first), np.array(values, dtype=np.float64))

    def table_uploaded(self):
        whole = self.numbers.size > self.lut_cap
        super().table_uploaded()
        if whole:
            self.dev = self.numbers.copy()
        elif self.last is not None:
            first, values = self.last
            self.dev = np.concatenate([self.dev, np.full(self.numbers.size - self.dev.size, np.nan)])
            self.dev[first:first + values.size] = values
        self.last = None

    def numbers_seen(self):
        return self.dev


class CodesGrowResetsLut(RefIndex):
    """21. a growing code column resets the LUT's length to 0"""

    def set_codes(self, first, codes):
        if self.col_len and int(first) + len(codes) > self.col_len:
            self.numbers = np.zeros(0)
        super().set_codes(first, codes)


NEW_INDEX_MUTANTS = {13: GroupedIgnoresLive, 14: GroupedSideSkipsFlush, 15: GroupedKeepsRowMasks, 16: RecommendResolvesEarly,
                     17: RecommendFoldsOldRow, 18: RecommendStrikesOnce, 19: RegrowDropsLut, 20: LutDirtyLastCall, 21: CodesGrowResetsLut}
INDEX_MUTANTS = {1: LostRemove, 2: StagedInvisibleOnce, 3: IdsNotMoved, 4: GrowForgetsTombstones, 5: SampleKeyCollision,
                 6: TiesByPosition, 7: StaleZeroFlag, 8: ByIdGathersOldRow, 9: TotalCountsDead, 10: CodesLostAfterDistinct,
                 12: RefillKeepsNorms}


# -- the mutants of the three composed reads: one stale-state defect each, on the state those reads lean on
class BestVetoStaleRanks(RefIndex):
    """24. recommend by best: the veto resolves a candidate id through the id-order table (d_rank2row), and an add does not clear
    rank_valid -- the table is the one built before the adds since the last compaction, so an id added (or written again) since
    then resolves to the row of its lower neighbour in id order (or to its own old row)"""

    table = None

    def on_compact(self, shrink):
        self.table = None

    def on_reset(self):
        self.table = None

    def veto_vector(self, id):
        if self.table is None:
            at = np.nonzero(self.alive)[0]
            order = np.argsort(self.ids[at], kind="stable")
            self.table = (self.ids[at][order], at[order])
        tids, trows = self.table
        j = max(int(np.searchsorted(tids, U64(id), side="right")) - 1, 0)
        return self.rows[min(int(trows[j]), self.n_rows() - 1)]


class BestVetoFirstRow(RefIndex):
    """25. recommend by best: among the rows that carry a candidate's id the veto takes the FIRST one, not the live one -- after a
    re-add or an upsert dn and the veto come from the superseded vector (until a compaction drops it)"""

    def veto_vector(self, id):
        return self.rows[np.nonzero(self.ids == U64(id))[0][0]]


class BestResolvesEarly(RecommendResolvesEarly):
    """26. recommend by best: the examples' rows are resolved (id2row) BEFORE the flush -- and the compaction inside it -- of the
    same read: every example is whatever sits at its old row number (the analogue of 16)"""


class BestScanForgetsLive(RefIndex):
    """27. recommend by best: the exact scan's own eligibility mask is the caller's mask alone, without the live bits -- a
    removed row is scored, kept and returned by a request that ends in the scan (until a compaction drops it)"""

    def stage_block(self, stage, mask):
        if stage != rbd.STAGE_SCAN:
            return self.block(mask)
        rows, ids, alive = self.seen()
        ok = self.ok_by_id(mask)
        keep = np.ones(len(ids), dtype=bool) if ok is None else ok_of_ids(ok, ids)
        return np.ascontiguousarray(rows[keep]), np.ascontiguousarray(ids[keep])

    def veto_vector(self, id):
        return self.rows[np.nonzero(self.ids == U64(id))[0][-1]]


class BestStageOneUnmasked(RefIndex):
    """28. recommend by best: the second list search (depth 1024) runs without the caller's mask, which was staged for the first"""

    def stage_block(self, stage, mask):
        return self.block(None if stage == 1 else mask)


class MmrRowsOneCompactionOld(RefIndex):
    """29. MMR: the host's id -> row map is not rebuilt by a compaction (only by adds and removes) -- the pair distances are read
    from the rows the candidates had BEFORE the rows moved; ids and query distances still look right"""

    snap = None

    def on_compact(self, shrink):
        if self.snap is None:
            self.snap = (self.ids.copy(), self.alive.copy())

    def _kill(self, ids):
        self.snap = None
        super()._kill(ids)

    def mmr_vectors(self, ids):
        if self.snap is None:
            return super().mmr_vectors(ids)
        sids, salive = self.snap
        return np.stack([self.rows[min(int(np.nonzero(salive & (sids == U64(i)))[0][-1]), self.n_rows() - 1)] for i in ids])


class MmrPairsOldRow(ByIdGathersOldRow):
    """30. MMR: the pair distances of an upserted id use its superseded row (the search itself, and search by id, are right)"""

    def vector_of(self, id):
        return RefIndex.vector_of(self, id)

    def mmr_vectors(self, ids):
        return np.stack([self.before.get(int(i), RefIndex.vector_of(self, i)) for i in ids])


class PerGroupStaleColumn(RefIndex):
    """31. per group: the member listing reads the code column as of the PREVIOUS upload (a distinct or per-group read): a
    set_codes since then reaches the search by group, not the listing"""

    column = None

    def listing_codes(self):
        return self.codes if self.column is None else self.column

    def distinct(self, *a, **kw):
        try:
            return super().distinct(*a, **kw)
        finally:
            self.column = self.codes.copy()

    def per_group(self, *a, **kw):
        try:
            return super().per_group(*a, **kw)
        finally:
            self.column = self.codes.copy()


class PerGroupListsTombstones(RefIndex):
    """32. per group: the member listing forgets the live bit -- a removed row of a wanted code is listed, ranked and returned
    (until a compaction drops it)"""

    def listing_block(self, mask):
        rows, ids, alive = self.seen()
        ok = self.ok_by_id(mask)
        keep = np.ones(len(ids), dtype=bool) if ok is None else ok_of_ids(ok, ids)
        return np.ascontiguousarray(rows[keep]), np.ascontiguousarray(ids[keep])


class GiantsDropMask(RefIndex):
    """33. per group: the giants' route searches under "code == c" alone and drops the caller's mask"""

    def giant_block(self, mask):
        return self.block(None)


class SwitchesRevertOnGrow(RefIndex):
    """34. the two debug switches live in the store's header: a re-allocation (a capacity doubling) puts debug_set_per_group_scan_cap
    and debug_set_recommend_best_route back to their defaults -- the answers stay, the counters show another route"""

    def on_grow(self):
        if self.cap:
            self.pg_cap = self.rb_route = 0


TWELVE_INDEX_MUTANTS = {24: BestVetoStaleRanks, 25: BestVetoFirstRow, 26: BestResolvesEarly, 27: BestScanForgetsLive, 28: BestStageOneUnmasked,
                        29: MmrRowsOneCompactionOld, 30: MmrPairsOldRow, 31: PerGroupStaleColumn, 32: PerGroupListsTombstones,
                        33: GiantsDropMask, 34: SwitchesRevertOnGrow}


# ---------------------------------------------------------------------------------------------------------------- the store
def flt_of(vdb, spec):
    """a filter as plain data -> MetadataFilter: ("eq" | "ne", field, value), ("exists", field), ("and" | "or", [specs]),
    ("lt" | "le" | "gt" | "ge", field, number -- or "-inf" / "inf", which a trace can print)"""
    if spec is None:
        return None
    F = vdb.MetadataFilter
    if spec[0] in ("and", "or"):
        return (F.And if spec[0] == "and" else F.Or)([flt_of(vdb, s) for s in spec[1]])
    return {"eq": F.Eq, "ne": F.Ne, "exists": F.Exists, "lt": F.Lt, "le": F.Le, "gt": F.Gt, "ge": F.Ge}[spec[0]](*spec[1:])


def spec_matches(spec, fields, number_of):
    """MetadataFilter.matches restated over a filter as plain data, with the numbers of the numeric leaves looked up by
    number_of(field, string) -> float or None: what the store mutants of the LUT change"""
    op = spec[0]
    if op == "and":
        return all(spec_matches(s, fields, number_of) for s in spec[1])
    if op == "or":
        return any(spec_matches(s, fields, number_of) for s in spec[1])
    have = fields.get(spec[1])
    if op == "exists":
        return have is not None
    if op == "eq":
        return have is not None and have == spec[2]
    if op == "ne":
        return have != spec[2]
    v = number_of(spec[1], have) if have is not None else None
    c = float(spec[2])
    return v is not None and {"lt": v < c, "le": v <= c, "gt": v > c, "ge": v >= c}[op]


class StoreSim:
    """VectorStore's semantics over anything with the index interface: string id -> (internal id, Metadata), an upsert removes the
    old internal id and adds the row under the next one, filters by MetadataFilter.matches over the live entries (never by any
    column).  stale_presence: mutant 11, the presence bit of a superseded internal id stays set, so a pre-filtered search still
    finds the old version.  lut: the two store mutants of the device table's numeric LUT -- "stale_sent" (22: _lut_sent survives
    set_device_filter(False) / (True), so the new table never receives the numbers of the dictionary values the old one had) and
    "bulk_only" (23: the numbers of new dictionary values are forwarded on a bulk attach only, not on single inserts).  Both
    show while the device filter is on and nowhere else: a numeric leaf then sees no number for such a value."""

    GROUP_FIELD = "grp"

    def __init__(self, vdb, index, stale_presence=False, lut=None):
        self.vdb, self.index, self.stale, self.lut = vdb, index, stale_presence, lut
        self.words, self.known, self.was_on = {}, {}, False          # field -> every value ever stored | those the table has numbers for
        self.entries, self.next, self.table = {}, 0, False           # sid -> (internal, Metadata)
        self.group_code = {}
        self.ghosts = {}                                             # internal -> (sid, Metadata) of superseded versions (mutant 11)

    def insert(self, sid, v, fields):
        old = self.entries.get(sid)
        if old is not None:
            if self.stale:
                self.ghosts[old[0]] = (sid, old[1], self.index.rows[np.nonzero(self.index.ids == U64(old[0]))[0][-1]].copy())
            self.index.remove(old[0])
        internal, self.next = self.next, self.next + 1
        self.index.add(internal, v)
        self.entries[sid] = (internal, self.vdb.Metadata(dict(fields)))
        for f, value in dict(fields).items():
            self.words.setdefault(f, set()).add(value)
            if self.table and self.lut != "bulk_only":
                self.known.setdefault(f, set()).add(value)
        g = dict(fields).get(self.GROUP_FIELD)
        self.index.set_codes(internal, [-1 if g is None else self.group_code.setdefault(g, len(self.group_code))])

    def delete(self, sid):
        e = self.entries.pop(sid, None)
        if e is None:
            raise Predicted("VectorNotFound", sid)
        self.index.remove(e[0])

    def compact(self):
        return self.index.compact()

    def set(self, name, value):
        if name == "device_filter":
            if value and not self.table:                             # a new table takes every column's numbers
                stale = self.lut == "stale_sent" and self.was_on
                self.known = {f: set() if stale else set(w) for f, w in self.words.items()}
                self.was_on = True
            self.table = bool(value)
        self.index.set(name, value)

    def _ok(self, spec):
        """eligibility by internal id of a pre-filter"""
        if spec is None:
            return None
        flt = flt_of(self.vdb, spec)
        ok = np.zeros(max(self.next, 1), dtype=bool)
        if self.lut and self.table:
            num = self.vdb.storage.num
            number_of = lambda f, s: num(s) if s in self.known.get(f, ()) else None
            for sid, (internal, meta) in self.entries.items():
                ok[internal] = spec_matches(spec, meta.fields(), number_of)
            return ok
        for sid, (internal, meta) in self.entries.items():
            ok[internal] = flt.matches(meta)
        return ok

    def _mask(self, spec):
        ok = self._ok(spec)
        return None if ok is None else ("host", ok)

    def _named(self, lists):
        name = {internal: sid for sid, (internal, _) in self.entries.items()}
        for internal, (sid, _, _) in self.ghosts.items():
            name.setdefault(internal, sid)
        return [[(name.get(int(i), f"?{int(i)}"), int(b)) for i, b in zip(*l)] for l in lists]

    def _empty(self):
        return not self.entries

    def _pre(self, read, *args, spec=None):
        """a pre-filtered read; mutant 11 adds the superseded versions that match the filter back for its duration"""
        mask = self._mask(spec)
        back = []
        if self.stale and spec is not None and self.ghosts:
            flt = flt_of(self.vdb, spec)
            back = [(i, g) for i, g in self.ghosts.items() if flt.matches(g[1])]
            for i, g in back:
                self.index.add(i, g[2])
                mask[1][i] = True
        try:
            return read(*args, mask)
        finally:
            for i, _ in back:
                self.index.remove(i)

    def search(self, q, k):
        return [] if self._empty() else self._named(self.index.search(q[None, :], int(k))["lists"])[0]

    def search_with_filter(self, q, k, spec):
        if self._empty():
            return []
        flt = flt_of(self.vdb, spec)
        meta = {internal: (sid, m) for sid, (internal, m) in self.entries.items()}
        fetch = min(max(3 * k, k), len(self.entries))
        ids, bits = self.index.search(q[None, :], fetch)["lists"][0]
        out = [(meta[int(i)][0], int(b)) for i, b in zip(ids, bits) if flt.matches(meta[int(i)][1])]
        return out[:k]

    def search_batch_prefiltered(self, q, ks, spec):
        return [[] for _ in q] if self._empty() else self._named(self._pre(self.index.search, q, ks, spec=spec)["lists"])

    def search_within(self, q, radius, limit, spec):
        if self._empty():
            return []
        return self._named(self._pre(self.index.range, q[None, :], [radius], limit, spec=spec)["lists"])[0]

    def search_similar_batch(self, sids, k, spec):
        ids = []
        for sid in sids:
            if sid not in self.entries:
                raise Predicted("VectorNotFound", sid)
            ids.append(self.entries[sid][0])
        return self._named(self._pre(self.index.by_id, np.array(ids, dtype=U64), int(k), spec=spec)["lists"])

    def search_distinct_batch(self, q, k, spec):
        if not self.table:
            raise Predicted("NeedsTable")
        return [[] for _ in q] if self._empty() else self._named(self._pre(self.index.distinct, q, int(k), spec=spec)["lists"])

    def search_batch_with_filters(self, q, ks, specs):
        """in the reference's terms: search_batch_prefiltered query by query, each under its own filter (None: the plain search)"""
        return [self.search_batch_prefiltered(q[b:b + 1], [k_of(ks, b)], spec)[0] for b, spec in enumerate(specs)]

    def recommend_batch(self, requests, k, spec):
        """the host composition: names -> internal ids (an unknown name: VectorNotFound), the index's recommend under the pre-filter"""
        pos, neg = [], []
        for p, n in requests:
            for sid in list(p) + list(n):
                if sid not in self.entries:
                    raise Predicted("VectorNotFound", sid)
            pos.append([self.entries[s][0] for s in p])
            neg.append([self.entries[s][0] for s in n])
        return self._named(self._pre(lambda p_, n_, k_, m_: self.index.recommend(p_, n_, k_, m_), pos, neg, int(k), spec=spec)["lists"])

    # -- the three composed reads (store schedules with "twelve": True)
    def search_mmr(self, q, k, lam, m, spec):
        """VectorStore.search_mmr: the index's MMR under the pre-filter; the store returns ids and query distances, no scores"""
        if self._empty():
            return []
        got = self._pre(lambda q_, k_, m_, l_, mk: self.index.mmr(q_, k_, m_, l_, mk), q[None, :], int(k), int(m), float(lam), spec=spec)
        named = self._named(got["lists"])[0]
        if "moved" not in got:
            return named
        return {"lists": [([s for s, _ in named], [b for _, b in named])], "moved": got["moved"]}   # (the model's: as_answer's form, and the cap's figure)

    def search_groups(self, q, k, g, spec):
        """VectorStore.search_groups over GROUP_FIELD: [(field value or None, members)] flattened to one list -- a header
        ("#value", size) in front of every group's (name, distance bits) entries -- so that diff() compares values, sizes and members"""
        if self._empty():
            return []
        value = {c: v for v, c in self.group_code.items()}
        got = self._pre(lambda q_, k_, g_, mk: self.index.per_group(q_, k_, g_, mk), q[None, :], int(k), int(g), spec=spec)["groups"][0]
        out = []
        for code, ids, bits in got:
            out.append((f"#{value.get(int(code))}", len(ids)))
            out.extend(self._named([(ids, bits)])[0])
        return out

    def recommend_best_batch(self, requests, k, spec):
        pos, neg = [], []
        for p, n in requests:
            for sid in list(p) + list(n):
                if sid not in self.entries:
                    raise Predicted("VectorNotFound", sid)
            pos.append([self.entries[s][0] for s in p])
            neg.append([self.entries[s][0] for s in n])
        return self._named(self._pre(lambda p_, n_, k_, m_: self.index.best(p_, n_, k_, m_), pos, neg, int(k), spec=spec)["lists"])


# ---------------------------------------------------------------------------------------------------------------- the runner
READ_OPS = READS
STORE_READS = ("s_search", "s_with_filter", "s_prefiltered", "s_within", "s_similar", "s_distinct")
NEW_STORE_READS = ("s_recommend", "s_with_filters")                 # (schedules with "numeric": True only)
NEWER_STORE_READS = ("s_mmr", "s_groups", "s_recommend_best")       # (schedules with "twelve": True only)


def is_read(op):
    return op[0] in READ_OPS or op[0] in NEW_READS or op[0] in NEWER_READS or op[0] in STORE_READS or op[0] in NEW_STORE_READS or op[0] in NEWER_STORE_READS


def queries(seed, key, log, B, d):
    """gaussian queries, most of them next to a stored (alive or removed) row, so that exact duplicates meet in the answers"""
    rng = rng_of(seed, key, 2)
    q = rng.standard_normal((B, d)).astype(F32)
    if log.n_rows() and log.d == d:
        near = rng.random(B) < 0.7
        at = rng.integers(0, log.n_rows(), B)
        q[near] = log.rows[at[near]] + F32(0.05) * q[near]
        if log.metric == COSINE:
            q[~q.any(axis=1)] = F32(1.0)
    return np.ascontiguousarray(q, dtype=F32)


def mask_of(seed, op_mask, log):
    """the mask of a read as plain data -> None | ("host", ok by id) | ("compiled", code) | ("numeric", leaf, const, code).
    In a trace a numeric mask is ("numeric", leaf, const key): the constant is one of the numbers set at that moment, from the
    middle four fifths of them, so that ties at equality occur and most masks keep a share of the rows; one draw in ten is
    -inf (Gt, Ge) or +inf (Lt, Le): every number passes, NaN does not.  With no number set yet it is 0.0 (and the mask admits
    nothing; the comparison no number passes, Lt(-inf), stands in grouped reads: grouped_masks)."""
    if op_mask is None:
        return None
    how, key, share = op_mask
    if how == "compiled":
        return ("compiled", int(key))
    if how == "numeric":
        rng = rng_of(seed, share, 8)
        have = np.sort(log.numbers[np.isfinite(log.numbers)])
        r, at, code = rng.random(), rng.random(), int(rng.integers(0, 30))
        const = float(have[int((0.1 + 0.8 * at) * have.size)]) if have.size else 0.0
        if r < 0.1:                                                  # (the infinity every number passes: a read must return a row)
            const = float("inf") if key in ("lt", "le") else float("-inf")
        return ("numeric", str(key), const, code)
    return ("host", rng_of(seed, key, 3).random(max(log.id_bound, 1)) < share)


def ks_of(k):
    return int(k) if np.isscalar(k) else np.array(k, dtype=np.uintp)


def materialise(trace, op, model):
    """a read op -> (method name, positional arguments) for model and adapter alike"""
    seed, kind = trace["seed"], op[0]
    d = model.d or trace["d"]
    if kind in ("search", "masked", "sparse"):
        _, B, k, qkey, m = op
        return "search", (queries(seed, qkey, model, B, d), ks_of(k), mask_of(seed, m, model))
    if kind == "distinct":
        _, B, k, qkey, m = op
        return "distinct", (queries(seed, qkey, model, B, d), ks_of(k), mask_of(seed, m, model))
    if kind == "range":
        _, B, qkey, rank, maxr, m = op
        q = queries(seed, qkey, model, B, d)
        mask = mask_of(seed, m, model)
        radii = np.ones(B, dtype=F32)
        if model.ids.size and not model.misfits and not model.zero_live():
            live = model._live(mask)
            for b in range(B):
                r = model.ranking(q[b], live)
                if len(r[0]):
                    radii[b] = rd.radius_at(r, min(int(rank), len(r[0])))
        return "range", (q, radii, int(maxr), mask)
    if kind == "by_id":
        _, B, k, skey, absent, m = op
        rng = rng_of(seed, skey, 4)
        live = model.live_ids()
        ids = live[rng.integers(0, live.size, B)] if live.size else np.zeros(B, dtype=U64)
        if live.size:                                                # half of them among the ids written last (added, upserted, re-added)
            last = model.ids[model.alive][-48:]
            recent = rng.random(B) < 0.5
            ids[recent] = last[rng.integers(0, last.size, B)][recent]
            ids[0] = last[-1]                                        # and always the very last one
        if absent or not live.size:
            gone = np.setdiff1d(model.ids, live)
            ids[int(rng.integers(0, B))] = gone[int(rng.integers(0, gone.size))] if gone.size else U64(ID_LIMIT - 1)
        return "by_id", (ids, ks_of(k), mask_of(seed, m, model))
    if kind == "numeric":
        _, B, k, qkey, m = op
        return "search", (queries(seed, qkey, model, B, d), ks_of(k), mask_of(seed, m, model))
    if kind == "grouped":
        _, B, k, qkey, G, form, gkey = op
        return "grouped", (queries(seed, qkey, model, B, d), ks_of(k)) + grouped_masks(seed, gkey, model, B, G, form)
    if kind == "recommend":
        _, B, k, ekey, absent, m = op
        pos, neg = requests_of(seed, ekey, model, B, absent)
        return "recommend", (pos, neg, ks_of(k), mask_of(seed, m, model))
    if kind == "mmr":
        _, B, k, qkey, m, lkey, mask = op
        q = queries(seed, qkey, model, B, d)
        if model.n_live() and model.d == d:                          # query 0 lies next to the row written last: it is candidate 0 and pick 1
            q[0] = model.rows[np.nonzero(model.alive)[0][-1]] + F32(0.05) * q[0]
            if model.metric == COSINE and not q[0].any():
                q[0] = F32(1.0)
        return "mmr", (q, ks_of(k), int(m), lambdas_of(seed, lkey, B), mask_of(seed, mask, model))
    if kind == "per_group":
        _, B, k, qkey, g, mask = op
        return "per_group", (queries(seed, qkey, model, B, d), ks_of(k), int(g), mask_of(seed, mask, model))
    if kind == "best":
        _, B, k, ekey, absent, mask = op
        pos, neg = best_requests_of(seed, ekey, model, B, absent)
        return "best", (pos, neg, ks_of(k), mask_of(seed, mask, model))
    raise ValueError(kind)


LAMBDAS = (0.0, 0.3, 0.5, 0.7, 1.0)


def lambdas_of(seed, lkey, B):
    """the trade-off of an MMR read: one f32 for the batch (keys 0..4 name LAMBDAS outright), or one per query"""
    if 0 <= int(lkey) < len(LAMBDAS):
        return float(LAMBDAS[int(lkey)])
    rng = rng_of(seed, lkey, 14)
    if rng.random() < 0.5 or B == 1:
        return float(rng.choice(LAMBDAS[:4]))
    return np.array(rng.choice(LAMBDAS, B), dtype=F32)


def best_requests_of(seed, ekey, log, B, absent):
    """(positives, negatives) of a recommend-by-best read: per request 1 to 4 positives and 0 to 2 negatives from the live ids, half
    of them among the 48 ids written last, an id repeated or put on both sides one time in five.  Request 0 always has two
    positives or more and a negative.  When the row written last lies beside another live row x without being its copy (the op
    "near"), request 0 is ([x, x], [the id written last -- and the one before it, if that lies beside x too]): such negatives veto
    half or more of all rows, the nearest included, which is what sends a request on to list stage 1.  Else, when another live
    row holds the very bits of the row written last (an add or an upsert that copies a stored row, a duplicate of a bulk), that
    row's id is the first positive of request 0 -- the id written last is then the nearest candidate of a request with a
    negative, and the veto has to resolve it to its row.  `absent` puts a removed (or never stored) id at a random place."""
    rng = rng_of(seed, ekey, 15)
    live = log.live_ids()
    last = log.ids[log.alive][-48:]

    def draw(n):
        if not live.size:
            return [0] * n
        ids = live[rng.integers(0, live.size, n)]
        recent = rng.random(n) < 0.5
        ids[recent] = last[rng.integers(0, last.size, n)][recent]
        return [int(i) for i in ids]
    reqs = []
    for b in range(B):
        npos, nneg = int(rng.integers(1, 5)), int(rng.integers(0, 3))
        if b == 0:
            npos, nneg = max(npos, 2), max(nneg, 1)
        p, n = draw(npos), draw(nneg)
        if rng.random() < 0.2:
            side = n if n and rng.random() < 0.5 else p
            side[int(rng.integers(0, len(side)))] = p[int(rng.integers(0, len(p)))]
        reqs.append([p, n])
    if live.size:
        at = np.nonzero(log.alive)[0]
        twin = at[:-1][(log.rows[at[:-1]] == log.rows[at[-1]]).all(axis=1)]
        gap = ((log.rows[at[:-1]].astype(np.float64) - log.rows[at[-1]]) ** 2).sum(axis=1) if at.size > 1 else np.zeros(0)
        beside = at[:-1][(gap > 0) & (gap < 1.0)]
        if beside.size:
            x, vetoes = int(log.ids[beside[0]]), [int(log.ids[at[-1]])]
            if at.size > 2 and at[-2] != beside[0] and 0 < ((log.rows[at[-2]].astype(np.float64) - log.rows[beside[0]]) ** 2).sum() < 1.0:
                vetoes.append(int(log.ids[at[-2]]))
            reqs[0] = [[x, x], vetoes]
        elif twin.size:
            x, newest = int(log.ids[twin[0]]), int(log.ids[at[-1]])
            other = [int(i) for i in live[:3] if int(i) not in (x, newest)][:1]
            reqs[0][0][0] = x
            reqs[0] = [[x if i == newest else i for i in reqs[0][0]], [i for i in reqs[0][1] if i not in (x, newest)] or other]
    if absent or not live.size:
        gone = np.setdiff1d(log.ids, live)
        b = int(rng.integers(0, B))
        side = reqs[b][int(rng.integers(0, 2)) if reqs[b][1] else 0]
        side[int(rng.integers(0, len(side)))] = int(gone[int(rng.integers(0, gone.size))]) if gone.size else ID_LIMIT - 1
    return [p for p, _ in reqs], [n for _, n in reqs]


def grouped_masks(seed, gkey, log, B, G, form):
    """(group_of u32 [B], masks) of a grouped read.  G masks, all host masks (form "host": eligible shares from SPARSE_SHARE, 0.5,
    0.9) or all compiled on the table ("compiled": Ne leaves; "numeric": numeric leaves among them).  One read in four holds a mask
    with no eligible live row (a host mask that admits the removed ids only; compiled: a numeric leaf no number passes), one in
    four a mask no query references (the last one).  group_of is drawn per query, VDB_GROUP_NONE included; from B = 8 on two
    queries share a group and one is unfiltered."""
    rng = rng_of(seed, gkey, 9)
    bound = max(log.id_bound, 1)
    masks = []
    for g in range(G):
        if form == "host":
            masks.append(("host", rng.random(bound) < float(rng.choice((SPARSE_SHARE, 0.5, 0.9)))))
        elif form == "numeric" and rng.random() < 0.6:
            masks.append(mask_of(seed, ("numeric", str(rng.choice(LEAVES)), int(rng.integers(0, 1 << 30))), log))
        else:
            masks.append(("compiled", int(rng.integers(0, 30))))
    barren, spare = rng.random() < 0.25, rng.random() < 0.25 and G > 1
    if barren:
        if form == "host":
            ok = np.ones(bound, dtype=bool)
            live = log.live_ids()
            ok[live[live < U64(bound)].astype(np.int64)] = False
            masks[0] = ("host", ok)
        else:
            masks[0] = ("numeric", "lt", float("-inf"), 0)
    used = G - 1 if spare else G
    group_of = rng.integers(0, used + 1, B).astype(np.int64)
    group_of[rng.random(B) < 0.15] = used
    if B >= 8:
        group_of[0] = group_of[1] = int(rng.integers(0, used))
        group_of[2] = used
    group_of = np.where(group_of == used, GROUP_NONE, group_of).astype(np.uint32)
    return group_of, masks


def requests_of(seed, ekey, log, B, absent):
    """(positives, negatives) of a recommend read: per request 1 to 8 positives and 0 to 4 negatives from the live ids, half of
    them among the 48 ids written last, an id repeated within a request one time in five; one request of the batch is ([x], []);
    the very last id is the last example of the longest request (not the first of a fold: RecommendFoldsOldRow); `absent` puts a removed (or never stored) id at a random place."""
    rng = rng_of(seed, ekey, 10)
    live = log.live_ids()
    last = log.ids[log.alive][-48:]

    def draw(n):
        if not live.size:
            return [0] * n
        ids = live[rng.integers(0, live.size, n)]
        recent = rng.random(n) < 0.5
        ids[recent] = last[rng.integers(0, last.size, n)][recent]
        return [int(i) for i in ids]
    reqs = []
    for b in range(B):
        ex = draw(int(rng.integers(1, 9)) + int(rng.integers(0, 5)))
        npos = max(1, len(ex) - int(rng.integers(0, min(5, len(ex)))))
        if len(ex) > 1 and rng.random() < 0.2:
            ex[int(rng.integers(1, len(ex)))] = ex[int(rng.integers(0, len(ex)))]
        reqs.append([ex[:npos], ex[npos:]])
    reqs[int(rng.integers(0, B))] = [draw(1), []]
    b = int(np.argmax([len(p) + len(n) for p, n in reqs]))             # the very last id: the last example of the longest request
    if live.size:
        reqs[b][1 if reqs[b][1] else 0][-1] = int(last[-1])
    if absent or not live.size:
        gone = np.setdiff1d(log.ids, live)
        b = int(rng.integers(0, B))
        side = reqs[b][int(rng.integers(0, 2)) if reqs[b][1] else 0]
        side[int(rng.integers(0, len(side)))] = int(gone[int(rng.integers(0, gone.size))]) if gone.size else ID_LIMIT - 1
    return [p for p, _ in reqs], [n for _, n in reqs]


def capture(call):
    try:
        return call()
    except Predicted as e:
        return {"error": (e.kind, e.id)}


def diff(want, got):
    """None, or what differs between two answers"""
    if "error" in want or "error" in got:
        return None if want.get("error") == got.get("error") else f"expected {want.get('error', 'an answer')}, got {got.get('error', 'an answer')}"
    if len(want["lists"]) != len(got["lists"]):
        return f"{len(want['lists'])} queries expected, {len(got['lists'])} answered"
    for b, (w, g) in enumerate(zip(want["lists"], got["lists"])):
        if len(w[0]) != len(g[0]):
            return f"query {b}: count {len(g[0])}, expected {len(w[0])}"
        if not np.array_equal(w[0], g[0]):
            at = int(np.nonzero(np.asarray(w[0]) != np.asarray(g[0]))[0][0])
            return f"query {b}: id {g[0][at]} at rank {at}, expected {w[0][at]}"
        if not np.array_equal(w[1], g[1]):
            at = int(np.nonzero(np.asarray(w[1]) != np.asarray(g[1]))[0][0])
            return f"query {b}: distance bits {g[1][at]:#x} at rank {at}, expected {w[1][at]:#x}"
    if "totals" in want and [int(t) for t in want["totals"]] != [int(t) for t in got["totals"]]:
        return f"range totals {list(map(int, got['totals']))}, expected {list(map(int, want['totals']))}"
    if "codes" in want and "codes" in got:
        for b, (w, g) in enumerate(zip(want["codes"], got["codes"])):
            if not np.array_equal(w, g):
                return f"query {b}: group codes {g}, expected {w}"
    for key in ("scores", "dn"):                                     # MMR's score bits, the dn bits of recommend by best score
        if key in want and key in got:
            for b, (w, g) in enumerate(zip(want[key], got[key])):
                if not np.array_equal(w, g):
                    return f"query {b}: {key} bits {[hex(int(x)) for x in g]}, expected {[hex(int(x)) for x in w]}"
    if "groups" in want and "groups" in got:                         # per group: the codes, the sizes, every member's id and distance bits
        for b, (w, g) in enumerate(zip(want["groups"], got["groups"])):
            if len(w) != len(g):
                return f"query {b}: {len(g)} groups, expected {len(w)}"
            for j, ((wc, wi, wd), (gc, gi, gd)) in enumerate(zip(w, g)):
                if int(wc) != int(gc) or not np.array_equal(wi, gi) or not np.array_equal(wd, gd):
                    return f"query {b}, group {j}: code {int(gc)} members {list(map(int, gi))} bits {[hex(int(x)) for x in gd]}, expected code {int(wc)} members {list(map(int, wi))} bits {[hex(int(x)) for x in wd]}"
    for key in ("struck", "cut", "stages", "gstats", "rstats", "mstats", "pstats", "bstats"):   # the engine's own counters of the read, where both sides have them
        if key in want and key in got and want[key] != got[key]:
            return f"{key} {got[key]}, expected {want[key]}"
    return None


def resolve(trace, op, log):
    """one non-read op of an index-level trace -> the concrete calls [(method, args)] it stands for, given the model's state
    (a duplicate of a stored row, remove_many and reset name no vector and no id themselves)"""
    seed, kind = trace["seed"], op[0]
    d = log.d or trace["d"]
    if kind in ("add", "upsert", "readd"):
        _, id, key, dup_of = op
        v = vectors(seed, key, 1, d)[0]
        at = np.nonzero(log.alive & (log.ids == U64(dup_of)))[0] if dup_of >= 0 else ()
        return [("add", (int(id), log.rows[at[-1]].copy() if len(at) else v))]
    if kind == "near":                                               # a row beside a stored one: as a negative it vetoes about half of ALL rows,
        _, id, key, of = op                                          # the nearest included (best_requests_of) -- a copy would veto every row
        at = np.nonzero(log.alive & (log.ids == U64(of)))[0]
        x, step = log.rows[at[-1]].astype(np.float64), vectors(seed, key, 1, d)[0].astype(np.float64)
        step -= (step @ x) / max(x @ x, 1e-30) * x                   # (at right angles to the row: the half of the rows it vetoes is a fair one)
        return [("add", (int(id), (x + 0.01 * step).astype(F32)))]
    if kind == "zero":
        return [("add", (int(op[1]), np.zeros(d, dtype=F32)))]
    if kind == "inf":                                                # one infinite element: the forward conversion of the rows refuses it
        v = vectors(seed, op[2], 1, d)[0]
        v[3] = np.inf
        return [("add", (int(op[1]), v))]
    if kind == "misfit":
        return [("add", (int(op[1]), np.ones(int(op[2]), dtype=F32)))]
    if kind in ("bulk", "reset"):
        _, n, d, base, perm, key, dup = op
        calls = [("remove", (log.live_ids(),))] if kind == "reset" and log.n_live() else []
        return calls + [("add_bulk", (vectors(seed, key, n, d, dup), bulk_ids(seed, key, n, base, perm)))]
    if kind in ("remove", "remove_absent"):
        return [("remove", (np.array([op[1]], dtype=U64),))]
    if kind == "remove_many":
        _, count, key = op
        live = log.live_ids()
        take = rng_of(seed, key, 5).permutation(live.size)[:max(0, min(int(count), live.size - 1))]
        return [("remove", (live[np.sort(take)],))] if take.size else []
    if kind in ("compact", "compact_shrink"):
        return [("compact", (kind == "compact_shrink",))]
    if kind == "auto_compact":
        return [("set_auto_compact", (float(op[1]),))]
    if kind == "codes":
        _, first, n, key, groups = op
        return [("set_codes", (int(first), rng_of(seed, key, 6).integers(-1, groups, n).astype(I32)))]
    if kind == "set":
        return [("set", (op[1], op[2]))]
    if kind == "flush":
        return [("flush", ())]
    if kind == "numbers":                                            # gaussians; NaN ("no number"), +0.0, -0.0 and exact duplicates among them
        _, first, n, key = op
        rng = rng_of(seed, key, 11)
        v = rng.standard_normal(n)
        r = rng.random(n)
        copy = r < 0.15
        v[copy] = v[rng.integers(0, n, n)][copy]
        v[(r >= 0.15) & (r < 0.2)] = 0.0
        v[(r >= 0.2) & (r < 0.25)] = -0.0
        v[(r >= 0.25) & (r < 0.35)] = np.nan
        return [("set_numbers", (int(first), v))]
    raise ValueError(kind)


def apply_mutation(trace, op, log):
    for name, args in resolve(trace, op, log):
        getattr(log, name)(*args)


def run(trace, adapter, expected=None, on_read=None):
    """Apply the trace to the adapter and to a fresh model; compare after every read (and the error of every mutation).
    expected: a list with one slot per op that keeps the reads' arguments and the model's answers between runs of one trace.
    on_read(step, op, model, args, got): called after every matching read.  Returns the model."""
    store = trace.get("store", False)
    model = StoreSim(adapter.vdb, Model(trace["metric"])) if store else Model(trace["metric"], sharded=getattr(adapter, "sharded", False))
    log = model_log(model)
    ops = trace["ops"]
    for step, op in enumerate(ops):
        what = None
        if not is_read(op):
            for name, args in (resolve_store(trace, op) if store else resolve(trace, op, log)):
                want = capture(lambda: getattr(model, name)(*args) and None or {})
                got = capture(lambda: getattr(adapter, name)(*args) and None or {})
                if want.get("error") != got.get("error"):
                    what = f"{name}: expected {want.get('error', 'no error')}, got {got.get('error', 'no error')}"
                    break
        else:
            if expected is not None and expected[step] is not None:
                name, args, want = expected[step]
                if log.sharded and name in NEWER_READS:              # refused -- or, by MMR and per group, an empty index answered first
                    want = capture(lambda: getattr(model, name)(*args))
                elif "error" not in want and not (name in ("range", "grouped") and log.sharded):
                    log.uploaded()                                   # (a refused read uploads nothing: as on the uncached path)
            else:
                name, args = materialise_store(trace, op, model) if store else materialise(trace, op, model)
                want = capture(lambda: getattr(model, name)(*args))
                if expected is not None and not log.sharded:
                    expected[step] = (name, args, want)
            if name in ("range", "grouped") and log.sharded:
                want = {"error": ("Refused", None)}
            if not store and compiles(name, args):
                log.table_uploaded()                                 # (the adapter compiles before it calls: also when the read fails)
            got = capture(lambda: getattr(adapter, name)(*args))
            if store:
                want, got = as_answer(want), as_answer(got)
            what = diff(want, got)
            if what is None and on_read is not None:
                on_read(step, op, model, args, got)
        if what is not None:
            head = {k: v for k, v in trace.items() if k != "ops"}
            head["ops"] = list(ops[:step + 1])
            raise Mismatch(f"seed {trace['seed']}, profile {trace.get('profile')}, step {step} {op}: {what}\n"
                           f"replay with lifecycle.run(TRACE, adapter), TRACE = {head!r}")
    return model


def compiles(name, args):
    """does this read compile a mask on the table (the table's staged writes are uploaded then)"""
    masks = args[3] if name == "grouped" else [args[-1]]
    return any(on_table(m) for m in masks)


def model_log(model):
    return model.index if isinstance(model, StoreSim) else model


def as_answer(x):
    """a store answer (a list of (sid, bits), or a list of such lists) in the form diff() compares"""
    if isinstance(x, dict):
        return x
    if x and isinstance(x[0], tuple) or not x:
        x = [x]
    return {"lists": [([s for s, _ in l], [b for _, b in l]) for l in x]}


def shrink(trace, make_adapter, log=None):
    """Drop ops greedily while the failure persists; make_adapter() gives a fresh adapter for every attempt.  Returns the
    smallest failing trace found (the failing read stays last)."""
    def fails(ops):
        t = dict(trace, ops=ops)
        try:
            run(t, make_adapter())
        except Mismatch as e:
            return int(str(e).split("step ")[1].split(" ")[0]) + 1
        except Exception:
            return 0                                                 # another failure than the one being shrunk: not this trace
        return 0
    ops = list(trace["ops"])
    n = fails(ops)
    if not n:
        return None
    ops = ops[:n]
    chunk = max(1, len(ops) // 4)
    while chunk >= 1:
        i = len(ops) - 1 - chunk
        while i >= 0:
            cand = ops[:i] + ops[i + chunk:]
            n = fails(cand)
            if n:
                ops = cand[:n]
                if log:
                    log(f"  {len(ops)} ops")
            i -= chunk
        chunk //= 2
    return dict(trace, ops=ops)


# ---------------------------------------------------------------------------------------------------------------- store traces
def store_vector(trace, key):
    return vectors(trace["seed"], key, 1, trace["d"])[0]


def doc_fields(trace, j, key):
    """the metadata of version `key` of document j: a group (absent for every 7th document), a parity that changes between versions"""
    f = {"par": str(int(rng_of(trace["seed"], key, 7).integers(0, 3))), "ver": str(key % 5)}
    if j % 7:
        f["grp"] = f"g{j % trace.get('groups', 40)}"
    if trace.get("numeric"):
        # ts: a decimal string of its own for nearly every version (the dictionary grows on almost every insert), now and then
        # one of the hard ones of tests/golden/numeric_strings.tsv; price: about 20 values, absent for every fifth document
        f["ts"] = TS_SPECIAL[key // 13 % len(TS_SPECIAL)] if key % 13 == 0 else str(key * 7919 % 1000003)
        if j % 5:
            f["price"] = f"{(key * 31 + j) % 20}.5"
    return f


TS_SPECIAL = ("-0", "1e400", "n/a", "007", "9007199254740993")


def resolve_store(trace, op):
    kind = op[0]
    if kind == "s_insert":
        _, j, key, dup_of = op
        return [("insert", (f"doc{j}", store_vector(trace, key if dup_of < 0 else dup_of), doc_fields(trace, j, key)))]
    if kind == "s_insert_many":                                      # every 9th document of the run shares one vector
        _, first, n, key = op
        return [("insert", (f"doc{j}", store_vector(trace, key * 100003 + (j if j % 9 else first)), doc_fields(trace, j, key * 100003 + j)))
                for j in range(first, first + n)]
    if kind in ("s_delete", "s_delete_absent"):
        return [("delete", (f"doc{op[1]}",))]
    if kind == "s_compact":
        return [("compact", ())]
    if kind == "set":
        return [("set", (op[1], op[2]))]
    raise ValueError(kind)


def materialise_store(trace, op, model):
    seed, kind, log = trace["seed"], op[0], model.index
    d = trace["d"]
    if kind == "s_search":
        return "search", (queries(seed, op[2], log, 1, d)[0], int(op[1]))
    if kind == "s_with_filter":
        return "search_with_filter", (queries(seed, op[2], log, 1, d)[0], int(op[1]), op[3])
    if kind == "s_prefiltered":
        _, B, k, qkey, spec = op
        return "search_batch_prefiltered", (queries(seed, qkey, log, B, d), ks_of(k), spec)
    if kind == "s_within":
        _, qkey, rank, limit, spec = op
        q = queries(seed, qkey, log, 1, d)[0]
        r = F32(1.0)
        if model.entries:
            ok = model._ok(spec)
            live = log._live(None if ok is None else ("host", ok))
            rank_ = log.ranking(q, live)
            if len(rank_[0]):
                r = rd.radius_at(rank_, min(int(rank), len(rank_[0])))
        return "search_within", (q, r, int(limit), spec)
    if kind == "s_similar":
        _, B, k, skey, spec, absent = op
        rng = rng_of(seed, skey, 4)
        names = sorted(model.entries)
        sids = [names[int(i)] for i in rng.integers(0, len(names), B)] if names else ["doc0"] * B
        if absent or not names:
            sids[int(rng.integers(0, B))] = "nobody"
        return "search_similar_batch", (sids, int(k), spec)
    if kind == "s_distinct":
        _, B, k, qkey, spec = op
        return "search_distinct_batch", (queries(seed, qkey, log, B, d), int(k), spec)
    if kind == "s_with_filters":                                     # a filter per query: some None, some structurally equal
        _, B, k, qkey, fkey = op
        rng = rng_of(seed, fkey, 12)
        pool = [NUMERIC_STORE_FILTERS[int(i)] for i in rng.integers(0, len(NUMERIC_STORE_FILTERS), 3)]
        specs = [None if rng.random() < 0.25 else pool[int(rng.integers(0, 3))] for _ in range(B)]
        return "search_batch_with_filters", (queries(seed, qkey, log, B, d), ks_of(k), specs)
    if kind == "s_mmr":
        _, k, qkey, lkey, m, spec = op
        return "search_mmr", (queries(seed, qkey, log, 1, d)[0], int(k), float(LAMBDAS[int(lkey)]), int(m), spec)
    if kind == "s_groups":
        _, k, qkey, g, spec = op
        return "search_groups", (queries(seed, qkey, log, 1, d)[0], int(k), int(g), spec)
    if kind == "s_recommend_best":
        _, B, k, rkey, spec, absent = op
        rng = rng_of(seed, rkey, 16)
        names = sorted(model.entries)
        pick = lambda n: [names[int(i)] for i in rng.integers(0, len(names), n)] if names else ["doc0"] * n
        reqs = [(pick(int(rng.integers(1, 4))), pick(int(rng.integers(0, 3)))) for _ in range(B)]
        if names:                                                    # request 0: two positives, one of them on both sides -- a veto that bites
            reqs[0] = (reqs[0][0][:1] + pick(1), reqs[0][0][:1])
        if absent or not names:
            reqs[int(rng.integers(0, B))][0][0] = "nobody"
        return "recommend_best_batch", (reqs, int(k), spec)
    if kind == "s_recommend":
        _, B, k, rkey, spec, absent = op
        rng = rng_of(seed, rkey, 13)
        names = sorted(model.entries)
        pick = lambda n: [names[int(i)] for i in rng.integers(0, len(names), n)] if names else ["doc0"] * n
        reqs = [(pick(int(rng.integers(1, 5))), pick(int(rng.integers(0, 3)))) for _ in range(B)]
        if absent or not names:
            reqs[int(rng.integers(0, B))][0][0] = "nobody"
        return "recommend_batch", (reqs, int(k), spec)
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------- the generator
PROFILES = {
    # d, the dimension after the reset, which error episodes it holds
    "even":   dict(d=64, d2=40, zero=True, misfit=False),
    "odd":    dict(d=40, d2=64, zero=True, misfit=False),
    "misfit": dict(d=40, d2=64, zero=True, misfit=True),
    "auto":   dict(d=64, d2=40, zero=True, misfit=False, auto=0.3),
}

# name, seed, profile, metric, what it is for
PINNED = (
    ("even-euclid", 11, "even", EUCLID, "ld % 64 == 0; grows 1024 -> 32768 rows of capacity, shrinks, collides the row count, resets to d = 40"),
    ("even-cosine", 12, "even", COSINE, "the same with a zero-norm episode: InvalidVector while the row lives, answers again once it is gone"),
    ("even-dot", 13, "even", DOT, "the same under Dot: negative radii, by-id lists that are cut rather than struck"),
    ("odd-euclid", 21, "odd", EUCLID, "ld % 64 != 0 (d = 40), reset to d = 64"),
    ("odd-cosine", 22, "odd", COSINE, "d = 40 with the zero-norm episode"),
    ("odd-dot", 23, "odd", DOT, "d = 40 under Dot"),
    ("misfit-euclid", 31, "misfit", EUCLID, "a row of another dimension comes and goes: DimensionMismatch from every read in between"),
    ("misfit-cosine", 32, "misfit", COSINE, "both error episodes in one life"),
    ("misfit-dot", 33, "misfit", DOT, "the misfit episode under Dot"),
    ("auto-euclid", 41, "auto", EUCLID, "auto-compaction on for most of the life: reads compact before they search"),
    ("auto-cosine", 42, "auto", COSINE, "auto-compaction with the zero-norm episode"),
    ("auto-dot", 43, "auto", DOT, "auto-compaction under Dot"),
)


class _Gen:
    def __init__(self, seed, profile, metric):
        self.p = dict(PROFILES[profile])
        self.trace = {"seed": int(seed), "profile": profile, "metric": int(metric), "d": self.p["d"], "ops": []}
        self.rng = np.random.default_rng([int(seed), 99])
        self.m = Model(metric)
        self.key = 0
        self.next_id = 0
        self.groups = 30
        self.last_mut = None
        self.pairs = set()
        self.turn = int(seed)
        self.distinct_seen = False

    def k(self):
        self.key += 1
        return self.key

    def emit(self, op):
        self.trace["ops"].append(op)
        if is_read(op):
            read_begins(self.trace, op, self.m)
            if self.last_mut:
                self.pairs.add((self.last_mut, op[0]))
                self.last_mut = None
        else:
            apply_mutation(self.trace, op, self.m)
            if op[0] in MUTATIONS12 or op[0] == "remove_many":
                self.last_mut = "remove" if op[0] == "remove_many" else op[0]

    # -- ids
    def fresh_ids(self, n):
        base, self.next_id = self.next_id, self.next_id + n
        assert self.next_id < ID_LIMIT - 1
        return base

    def live_id(self):
        live = self.m.live_ids()
        return int(live[int(self.rng.integers(0, live.size))])

    def dead_id(self):
        gone = np.setdiff1d(self.m.ids, self.m.live_ids())
        return int(gone[int(self.rng.integers(0, gone.size))]) if gone.size else None

    # -- reads
    def draw_k(self, B):
        r = self.rng.random()
        if r < 0.15 and B > 1:
            return tuple(int(x) for x in self.rng.choice(KS, B))
        return int(self.rng.choice(KS, p=(0.2, 0.45, 0.2, 0.15)))

    def draw_B(self):
        big = self.m.n_rows() > 9000
        return int(self.rng.choice(BATCHES, p=(0.4, 0.3, 0.25, 0.05) if big else (0.25, 0.3, 0.25, 0.2)))

    def draw_mask(self, allow_none=True, compiled=True):
        r = self.rng.random()
        if allow_none and r < 0.6:
            return None
        if r < 0.8 or not compiled:
            return ("host", self.k(), float(self.rng.choice((0.5, 0.9))))
        return ("compiled", int(self.rng.integers(0, self.groups)), 0.0)

    def read(self, kind=None, absent=False):
        if kind is None:
            after = self.last_mut
            want = [r for r in READS if after and (after, r) not in self.pairs]
            self.turn += 1
            kind = want[self.turn % len(want)] if want else READS[self.turn % len(READS)]
        B = self.draw_B()
        if kind == "search":
            self.emit(("search", B, self.draw_k(B), self.k(), None))
        elif kind == "masked":
            self.emit(("masked", B, self.draw_k(B), self.k(), self.draw_mask(False)))
        elif kind == "sparse":
            self.emit(("sparse", B, self.draw_k(B), self.k(), ("host", self.k(), SPARSE_SHARE)))
        elif kind == "range":
            rank = int(self.rng.choice((3, 40, 600, 2500)))
            self.emit(("range", B, self.k(), rank, int(self.rng.choice((8, 256, 2048))),
                       self.draw_mask(compiled=False) if self.rng.random() < 0.4 else None))   # (the range call takes a host mask only)
        elif kind == "by_id":
            self.emit(("by_id", B, self.draw_k(B), self.k(), bool(absent), None if self.rng.random() < 0.7 else self.draw_mask(False)))
        elif kind == "distinct":
            self.emit(("distinct", B, self.draw_k(B), self.k(), self.draw_mask() if self.rng.random() < 0.4 else None))

    # -- mutations
    def mutate(self, kind):
        rng, d = self.rng, self.m.d
        if kind == "add":
            dup = self.live_id() if rng.random() < 0.3 else -1
            self.emit(("add", self.fresh_ids(1), self.k(), dup))
        elif kind == "upsert":
            self.emit(("upsert", self.live_id(), self.k(), -1))
        elif kind == "readd":
            i = self.dead_id()
            if i is None:
                return self.mutate("upsert")
            self.emit(("readd", i, self.k(), -1))
        elif kind == "remove":
            if self.m.n_live() < 50:
                return self.mutate("add")
            if rng.random() < 0.5:
                self.emit(("remove", self.live_id()))
            else:
                self.emit(("remove_many", int(rng.integers(5, max(6, self.m.n_live() // 12))), self.k()))
        elif kind == "remove_absent":
            i = self.dead_id()
            self.emit(("remove_absent", i if i is not None and rng.random() < 0.5 else ID_LIMIT - 2 - int(rng.integers(0, 1000))))
        elif kind == "bulk":
            n = int(rng.integers(40, 400))
            if rng.random() < 0.3 and self.m.n_live() > n:                   # a bulk over ids that are live: an upsert of a range
                base = int(self.m.live_ids()[0])
            else:
                base = self.fresh_ids(n)
            self.emit(("bulk", n, d, base, int(rng.random() < 0.6), self.k(), 0.15))
        elif kind in ("compact", "compact_shrink"):
            self.emit((kind,))
        elif kind == "auto_compact":
            self.emit(("auto_compact", float(rng.choice((0.0, 0.1, 0.3, 0.6)))))
        elif kind == "codes":
            n = int(rng.integers(1, 600))
            first = int(rng.integers(0, max(1, self.m.id_bound)))
            self.emit(("codes", first, min(n, ID_LIMIT - first), self.k(), int(rng.choice((6, self.groups, 150)))))

    def toggle(self):
        rng = self.rng
        name = str(rng.choice(("shadow", "sample_cache", "screen", "tiers", "sparse_filter", "large_k", "bounce", "flush")))
        if name == "flush":
            self.emit(("flush",))
        elif name == "tiers":
            self.emit(("set", "tiers", int(rng.choice((0, NO_DIRECT)))))
        elif name == "sparse_filter":
            self.emit(("set", "sparse_filter", int(rng.choice((0, 1, 1, 2)))))
        elif name == "bounce":
            self.emit(("set", "bounce", int(rng.choice((0, 64, 512)))))
        else:
            self.emit(("set", name, int(rng.integers(0, 2))))

    def mix(self, steps, kinds=None):
        kinds = kinds or ("add", "add", "upsert", "upsert", "readd", "remove", "remove", "remove_absent", "bulk", "compact",
                          "compact_shrink", "auto_compact", "codes", "codes")
        for _ in range(steps):
            r = self.rng.random()
            if r < 0.15:
                self.toggle()
                continue
            self.turn += 1
            missing = [m for m in kinds if any((m, rd_) not in self.pairs for rd_ in READS)]
            kind = missing[self.turn % len(missing)] if missing and r < 0.75 else str(self.rng.choice(kinds))
            self.mutate(kind)
            if self.rng.random() < 0.85:
                self.read()
                if self.rng.random() < 0.25:
                    self.read()

    def bulk(self, n, d=None, perm=1):
        self.emit(("bulk", n, d or self.m.d or self.p["d"], self.fresh_ids(n), perm, self.k(), 0.15))

    def build(self):
        p, rng = self.p, self.rng
        sparse0 = int(rng.choice((1, 2)))
        self.emit(("set", "sparse_filter", sparse0))
        self.emit(("set", "shadow", 1))
        self.emit(("set", "bounce", 64))
        self.bulk(int(rng.integers(600, 900)), p["d"])
        self.emit(("codes", 0, 3000, self.k(), 6))                  # few groups: stage A is too shallow for most k
        self.read("distinct")
        # one read for each route a small index has, whatever the draws below bring: the direct path, dense scores, the exact scan
        # (k beyond the candidate depth), the sparse route, distinct stage B (113 groups are not among the first 452 ranks), by-id
        # lists that are cut (the own id masked out)
        self.emit(("set", "tiers", 0))
        self.emit(("set", "sparse_filter", 1))
        self.emit(("search", 8, 10, self.k(), None))
        self.emit(("search", 9, 10, self.k(), None))
        self.emit(("search", 9, 300, self.k(), None))
        self.emit(("sparse", 9, 10, self.k(), ("host", self.k(), SPARSE_SHARE)))
        self.emit(("distinct", 8, 113, self.k(), None))
        self.emit(("by_id", 40, 10, self.k(), False, ("host", self.k(), 0.5)))
        self.emit(("set", "sparse_filter", sparse0))
        self.mix(28)
        if p.get("auto"):
            self.emit(("auto_compact", p["auto"]))
            self.read()
        # grow through the doublings, a few reads on every level, single adds in between so that rows are staged when reads arrive
        for n in (1300, 2500, 4500):
            self.mutate("remove")                                   # dead rows in the store when it is re-allocated ...
            self.bulk(n)
            self.read("search")                                     # ... and a read right behind the doubling
            self.mix(4)
        self.emit(("set", "shadow", 1))                             # the store is re-allocated with the bf16 shadow in place
        self.bulk(SMALL_N - 300 - self.m.n_rows())                  # just below SMALL_N: the dense path at its largest
        self.mutate("add")
        self.read("search")
        self.bulk(1000)                                             # across SMALL_N upward
        self.mutate("add")
        self.read("search")
        self.emit(("set", "tiers", 0))
        self.emit(("search", 9, 10, self.k(), None))                # the fused f32 pass
        self.mix(7)
        self.emit(("set", "tiers", 0))
        self.read("masked")
        # back down: most rows go, rows are staged, the compaction takes them along
        self.emit(("auto_compact", 0.0))
        self.emit(("set", "bounce", 64))                            # wide gaps, a small buffer: chunks move directly
        self.emit(("remove_many", self.m.n_live() - 2600, self.k()))
        self.read()
        self.mutate("add")
        self.mutate("upsert")
        self.emit(("compact",))
        self.read()
        self.mix(6)
        # the row count collides: a read at n rows, a shrinking compaction, adds back to exactly n rows, a read
        self.emit(("compact",))
        self.read("search")
        n = self.m.n_rows()
        self.emit(("remove_many", 700, self.k()))
        self.emit(("set", "bounce", 0))                             # scattered dead rows, the default buffer: through the bounce buffer
        self.emit(("compact_shrink",))
        self.bulk(n - self.m.n_rows())
        self.read()
        self.read("search")
        self.mix(6)
        if p.get("auto"):
            self.emit(("auto_compact", p["auto"]))
        else:
            self.emit(("auto_compact", 0.25))
        self.emit(("remove_many", int(self.m.n_live() * 0.45), self.k()))
        self.read()
        if not p.get("auto"):
            self.emit(("auto_compact", 0.0))
        if p["zero"] and self.trace["metric"] == COSINE:
            z = self.fresh_ids(1)
            self.emit(("zero", z))
            self.read("search")
            self.read("by_id")
            self.emit(("remove", z))
            self.read("range")
            self.read("search")
        if p["misfit"]:
            z = self.fresh_ids(1)
            self.emit(("misfit", z, p["d"] + 3))
            self.read("distinct")
            self.read("search")
            self.emit(("remove", z))
            self.read("by_id")
        self.read("by_id", absent=True)
        self.mix(5)
        # everything goes; the refill has another dimension
        self.emit(("remove_many", max(0, self.m.n_live() - 300), self.k()))
        n = int(rng.integers(700, 1000))
        self.emit(("reset", n, p["d2"], self.fresh_ids(n), 1, self.k(), 0.15))
        self.read(READS[self.trace["seed"] % len(READS)])          # (the pinned seeds take every kind here)
        self.mix(22)
        self.bulk(1500)
        self.read()
        return self.trace


LARGE_ROWS = 75_000      # above BF16_MIN_ROWS = 65536 and above the large-k floor 240 (113 + 192) = 73200 rows

# The issue holds the schedules to 20 000 rows AND asks for the bf16 screen and both range routes, which start at 65 536 rows
# (32 768 survivors for the dense range fallback).  These three short schedules settle it: d = 64, few reads, small batches.
LARGE_PINNED = (
    ("large-euclid", 61, EUCLID, "the screening tier's state: grows past 65 536 rows with the shadow on, toggles shadow / sample cache / "
                                 "screen, shrink-compacts and refills to the same row count, reads plain, large-k and range"),
    ("large-cosine", 62, COSINE, "the same under Cosine"),
    ("large-dot", 63, DOT, "the same under Dot"),
)


def large_schedule(seed, metric):
    g = _Gen(seed, "even", metric)
    g.trace["profile"] = "large"
    e, k = g.emit, g.k

    def reads():                                                     # plain (bf16 screen), large k on the screening tier, both range routes
        e(("search", 9, 10, k(), None))
        e(("search", 1, 113, k(), None))
        e(("range", 8, k(), 40, 256, None))                          # the screened route: the candidates of a tight radius
        e(("range", 1, k(), 40_000, 2048, None))                     # more than 32 768 survivors: the dense fallback
    e(("set", "shadow", 1))
    e(("set", "sparse_filter", 1))
    g.bulk(900, 64)
    e(("codes", 0, 3000, k(), 6))
    for n in (20_000, 30_000, LARGE_ROWS - 50_900 - 1200):           # re-allocations with the shadow in place, across 65 536 rows
        g.bulk(n)
        e(("search", 1, 10, k(), None))                              # (a bulk is staged like a single add: the read uploads it, the store grows)
    g.mutate("add")
    reads()
    e(("by_id", 8, 10, k(), False, None))
    e(("distinct", 8, 10, k(), None))
    e(("masked", 8, 10, k(), ("host", k(), 0.5)))
    e(("sparse", 8, 10, k(), ("host", k(), SPARSE_SHARE)))
    for name, value in (("sample_cache", 0), ("sample_cache", 1), ("shadow", 0), ("screen", 0), ("screen", 1), ("shadow", 1), ("large_k", 0),
                        ("large_k", 1)):
        e(("set", name, value))
        g.mutate(("upsert", "add", "remove")[value + (name == "shadow")])
        e(("search", 9, 10, k(), None))
        e(("search", 1, 113, k(), None))
        if name in ("screen", "shadow"):
            e(("range", 8, k(), 40, 256, None))
    # the row count collides above the floor: reads at n rows, a shrinking compaction, adds back to exactly n rows, the reads again
    e(("compact",))
    reads()
    n = g.m.n_rows()
    e(("remove_many", 900, k()))
    e(("compact_shrink",))
    g.bulk(n - g.m.n_rows())
    reads()
    e(("by_id", 8, 10, k(), False, None))
    g.mutate("upsert")
    g.mutate("remove")
    reads()
    # back below the floor through removes and a compaction with rows staged, and up again
    e(("remove_many", g.m.n_live() - 60_000, k()))
    g.mutate("add")
    e(("compact",))
    e(("search", 9, 10, k(), None))
    e(("range", 8, k(), 40, 256, None))
    g.bulk(LARGE_ROWS - g.m.n_rows())
    reads()
    return g.trace


# ---------------------------------------------------------------------------------------------------------------- grouped, recommend, numeric
# Schedules of their own for the three read paths added after 266122c: the old traces are dealt from one rng stream each, so a
# new read kind in _Gen.read() would re-deal all of them.  The trace key "numbers" marks a schedule that holds them.
PROFILES["nine"] = dict(d=64, d2=40, zero=True, misfit=False)
PROFILES["nine-auto"] = dict(d=40, d2=64, zero=True, misfit=True, auto=0.3)

NEW_PINNED = (
    ("nine-euclid", 71, "nine", EUCLID, "all nine read kinds, the LUT set late and regrown twice; d = 64, reset to d = 40"),
    ("nine-cosine", 72, "nine", COSINE, "the same with the zero-norm episode: grouped and recommend fail while the row lives"),
    ("nine-dot", 73, "nine", DOT, "the same under Dot"),
    ("nine-auto-euclid", 81, "nine-auto", EUCLID, "d = 40, reset to d = 64, auto-compaction on: recommend compacts before it folds; a misfit episode"),
    ("nine-auto-cosine", 82, "nine-auto", COSINE, "auto-compaction with both error episodes"),
    ("nine-auto-dot", 83, "nine-auto", DOT, "auto-compaction under Dot"),
)


def carries_numeric(op):
    return op[0] == "grouped" and op[5] == "numeric" or op[0] != "grouped" and is_read(op) and op[-1] is not None and op[-1][0] == "numeric"


class _Gen9(_Gen):
    def __init__(self, seed, profile, metric):
        super().__init__(seed, profile, metric)
        self.trace["numbers"] = True
        self.used = Counter()

    def emit(self, op):
        if is_read(op):
            self.used[op[0]] += 1
        super().emit(op)

    def lut(self):
        return self.m.numbers.size

    def numeric_mask(self):
        return ("numeric", str(self.rng.choice(LEAVES)), self.k())

    def draw_mask9(self, after_numbers, none=0.6):
        r = self.rng.random()
        if after_numbers or (self.lut() and r > 0.75):
            return self.numeric_mask()
        if r < none:
            return None
        return self.draw_mask(False)

    def draw_grouped_k(self, B):
        if self.m.n_live() > GROUPED_MAX_K and self.rng.random() < 0.125:
            return GROUPED_BIG_K
        return self.draw_k(B)

    def read(self, kind=None, absent=False):
        after_numbers = self.last_mut == "numbers"
        if kind is None:                                             # a kind this mutation has not been followed by yet; the least used one
            after = self.last_mut
            want = [r for r in (NUMERIC_CARRIERS if after == "numbers" else NEW_READS) if after and (after, r) not in self.pairs]
            least = min(self.used[r] for r in READS9)
            want = [r for r in want if self.used[r] <= least + 2]    # (no kind runs away: every kind keeps its 8 % of the reads)
            kind = min(want or READS9, key=lambda r: (self.used[r], READS9.index(r)))
        if kind in ("search", "sparse", "range"):
            return super().read(kind)
        B = self.draw_B()
        if kind == "masked":
            self.emit(("masked", B, self.draw_k(B), self.k(), self.numeric_mask() if after_numbers else self.draw_mask(False)))
        elif kind == "numeric":
            self.emit(("numeric", B, self.draw_k(B), self.k(), self.numeric_mask()))
        elif kind == "by_id":
            self.emit(("by_id", B, self.draw_k(B), self.k(), bool(absent), self.draw_mask9(after_numbers, 0.7)))
        elif kind == "distinct":
            self.emit(("distinct", B, self.draw_k(B), self.k(), self.draw_mask9(after_numbers, 0.6)))
        elif kind == "grouped":
            r = self.rng.random()
            form = "numeric" if after_numbers or (self.lut() and r < 0.3) else "host" if r < 0.8 else "compiled"
            k, qkey, G = self.draw_grouped_k(B), self.k(), int(self.rng.integers(1, 7))
            for _ in range(20):                                      # a binding key under which some query has a row to return (a cap on the inputs)
                op = ("grouped", B, k, qkey, G, form, self.k())
                group_of, masks = materialise(self.trace, op, self.m)[1][2:]
                if any(g == GROUP_NONE or self.m._live(masks[int(g)]).any() for g in group_of):
                    break
            self.emit(op)
        elif kind == "recommend":                                    # an example key under which the read strikes or cuts an entry (a cap on the inputs)
            k, mask = self.draw_k(B), self.draw_mask9(after_numbers, 0.6)
            for _ in range(20):
                op = ("recommend", B, k, self.k(), bool(absent), mask)
                got = capture(lambda: self.m.recommend(*materialise(self.trace, op, self.m)[1]))
                if "error" in got or got["rstats"][1] or got["cut"]:
                    break
                if _ == 4:                                           # (B = 1 names the last id whatever the key: a copy of a row with a lower id
                    k = 10                                           # stands behind the cut of k = 1)
            self.emit(op)

    def mutate(self, kind):
        rng = self.rng
        if kind == "numbers":
            L = self.lut()
            if not L:
                return self.emit(("numbers", 0, self.groups + 1, self.k()))
            first = int(rng.integers(0, L))
            self.emit(("numbers", first, int(rng.integers(1, L - first + 1)), self.k()))
            if rng.random() < 0.5:                                   # a second call before the next compile: disjoint, or across the first
                lo = int(rng.integers(0, max(1, first)))
                self.emit(("numbers", lo, int(rng.integers(1, max(2, (first if rng.random() < 0.6 else L) - lo))), self.k()))
        elif kind == "codes":                                        # codes from a range wider than the LUT: some have no number
            n = int(rng.integers(1, 3000))
            first = int(rng.integers(0, max(1, self.m.id_bound)))
            self.emit(("codes", first, min(n, ID_LIMIT - first), self.k(), max(6, int(1.15 * self.lut()))))
        else:
            super().mutate(kind)

    def grouped_all(self, B, k, G):
        """a grouped read of G host masks whose binding key leaves no mask unreferenced and none without a live row: R = G"""
        live = self.m.live_ids().astype(np.int64)
        while True:
            key = self.k()
            group_of, masks = grouped_masks(self.trace["seed"], key, self.m, B, G, "host")
            if len(set(group_of.tolist()) - {GROUP_NONE}) == G and all(m[1][live].any() for m in masks):
                return self.emit(("grouped", B, k, self.k(), G, "host", key))

    def codes_all(self):
        self.emit(("codes", 0, self.m.id_bound, self.k(), max(self.groups, int(1.15 * self.lut()))))

    def extend_lut(self, to):
        """the LUT grows past its device capacity: overwrite a range, then the new tail; the next compile regrows the array"""
        L = self.lut()
        self.emit(("numbers", L // 2, L - L // 2, self.k()))
        self.emit(("numbers", L, to - L, self.k()))
        self.read("numeric")
        self.codes_all()
        self.read("masked")

    def mix(self, steps, kinds=None):
        kinds = kinds or ("add", "add", "upsert", "upsert", "readd", "remove", "remove", "remove_absent", "bulk", "compact",
                          "compact_shrink", "auto_compact", "codes", "codes", "numbers", "numbers")
        for _ in range(steps):
            r = self.rng.random()
            if r < 0.1:
                self.toggle()
                continue
            self.turn += 1
            missing = [m for m in kinds if any((m, rd_) not in self.pairs for rd_ in NEW_READS)]
            kind = missing[self.turn % len(missing)] if missing and r < 0.75 else str(self.rng.choice(kinds))
            self.mutate(kind)
            self.read()
            if self.rng.random() < 0.2:
                self.read()

    def build(self):
        p, rng, e, k = self.p, self.rng, self.emit, self.k
        e(("set", "sparse_filter", int(rng.choice((1, 2)))))
        e(("set", "shadow", 1))
        e(("set", "bounce", 64))
        self.bulk(int(rng.integers(600, 900)), p["d"])
        e(("codes", 0, 3000, k(), self.groups))
        # no LUT yet: every numeric leaf is false, the Ne masks and the unfiltered queries of the same batch answer
        e(("grouped", 9, 10, k(), 4, "numeric", k()))
        self.mutate("numbers")
        self.read("numeric")
        e(("numbers", 0, 10, k()))                                   # two disjoint writes, then one across both, before the next compile
        e(("numbers", 20, self.groups - 19, k()))
        self.read("numeric")
        e(("numbers", 3, 4, k()))
        e(("numbers", 5, 20, k()))
        e(("numbers", 0, 4, k()))
        self.read("masked")
        # two grouped reads of two masks each with a remove in between: the row count and the number of masks stay, the masks and
        # the live bits do not
        self.grouped_all(9, 113, 2)
        e(("remove_many", 60, k()))
        self.grouped_all(9, 113, 2)
        self.mutate("upsert")                                        # the upserted id is the last example of a longer request
        e(("recommend", 8, 10, k(), False, None))
        self.mutate("numbers")
        self.read("grouped")
        self.mutate("numbers")
        self.read("recommend")
        for kind in NEW_READS:                                       # (ids to re-add are rare later: a compaction forgets them)
            self.mutate("readd")
            self.read(kind)
        self.mix(22)
        if p.get("auto"):
            e(("auto_compact", p["auto"]))
            self.read()
        # grow through the doublings; a grouped read with unfiltered queries right behind a staged bulk, the LUT regrown on the way
        for n, lut, form in ((1300, 1300, "host"), (2500, 2600, "compiled"), (4500, 0, "numeric")):
            self.mutate("remove")
            self.bulk(n)
            e(("grouped", 9, 300, k(), 2, form, k()))
            if lut:
                self.extend_lut(lut)
            self.mix(2)
        e(("set", "shadow", 1))
        self.bulk(SMALL_N - 300 - self.m.n_rows())
        self.codes_all()
        self.mutate("add")
        self.read()
        self.bulk(1000)                                              # across SMALL_N upward
        self.mutate("add")
        self.grouped_all(8, GROUPED_BIG_K, 3)                        # k > 2048: one ordinary masked search per group, rows staged
        self.read()
        self.mix(4)
        # back down: most rows go, rows are staged, the compaction takes them along
        e(("auto_compact", 0.0))
        e(("set", "bounce", 64))
        e(("remove_many", self.m.n_live() - 2600, k()))
        self.read()
        self.mutate("add")
        self.mutate("upsert")
        e(("compact",))
        self.read()
        e(("compact_shrink",))
        self.read("grouped")
        self.mix(4)
        # the row count collides under grouped reads of the same number of masks
        e(("compact",))
        self.grouped_all(9, 10, 3)
        n = self.m.n_rows()
        e(("remove_many", 700, k()))
        e(("set", "bounce", 0))
        e(("compact_shrink",))
        self.bulk(n - self.m.n_rows())
        self.grouped_all(9, 10, 3)
        self.read()
        self.mix(4)
        # auto-compaction inside a recommend read: the examples resolve to the rows AFTER it
        e(("auto_compact", p.get("auto") or 0.25))
        e(("remove_many", int(self.m.n_live() * 0.45), k()))
        e(("recommend", 9, 10, k(), False, None))
        if not p.get("auto"):
            e(("auto_compact", 0.0))
        if p["zero"] and self.trace["metric"] == COSINE:
            z = self.fresh_ids(1)
            e(("zero", z))
            self.read("grouped")
            self.read("recommend")
            e(("remove", z))
            self.read("numeric")
        if p["misfit"]:
            z = self.fresh_ids(1)
            e(("misfit", z, p["d"] + 3))
            self.read("recommend")
            self.read("grouped")
            e(("remove", z))
            self.read("numeric")
        self.read("recommend", absent=True)
        self.mix(3)
        # everything goes; the refill has another dimension
        e(("remove_many", max(0, self.m.n_live() - 300), k()))
        n = int(rng.integers(700, 1000))
        e(("codes", 0, self.next_id + n, k(), max(self.groups, int(1.15 * self.lut()))))   # (the codes of the ids to come: the read behind the reset finds numbers)
        e(("reset", n, p["d2"], self.fresh_ids(n), 1, k(), 0.15))
        self.read(NEW_READS[self.trace["seed"] % 3])          # (the pinned seeds take every new kind here)
        self.mix(18)
        for m, r in [(m, r) for m in MUTATIONS12 for r in NEW_READS if m != "reset"]:   # what the draws left out, while the trace is short
            if (m, r) not in self.pairs and len(self.trace["ops"]) < 236:
                self.mutate(m)
                self.read(r)
        self.bulk(1500)
        self.read()
        return self.trace


# ---------------------------------------------------------------------------------------------------------------- MMR, per group, recommend by best
# Schedules of their own once more (TWELVE_PINNED), a generator class beside _Gen9 with an rng stream of its own: the 19 + 9 + 3
# older traces stay op for op what they are.  The trace key "twelve" marks a schedule that holds the three kinds.
PROFILES["twelve"] = dict(d=64, d2=40, zero=True, misfit=False)
PROFILES["twelve-auto"] = dict(d=40, d2=64, zero=True, misfit=True, auto=0.3)

TWELVE_PINNED = (
    ("twelve-euclid", 101, "twelve", EUCLID, "all twelve read kinds, both debug switches set mutations before they are read; d = 64, reset to d = 40"),
    ("twelve-cosine", 102, "twelve", COSINE, "the same with the zero-norm episode: the three composed reads fail while the row lives"),
    ("twelve-dot", 103, "twelve", DOT, "the same under Dot"),
    ("twelve-auto-euclid", 111, "twelve-auto", EUCLID, "d = 40 (ragged against the row pitch), reset to d = 64, auto-compaction on: the reads compact before they resolve ids; a misfit episode"),
    ("twelve-auto-cosine", 112, "twelve-auto", COSINE, "auto-compaction with both error episodes"),
    ("twelve-auto-dot", 113, "twelve-auto", DOT, "auto-compaction under Dot"),
)
BEST_KS = (1, 10, 113, 300)


class _Gen12(_Gen9):
    def __init__(self, seed, profile, metric):
        super().__init__(seed, profile, metric)
        self.trace["twelve"] = True
        self.rng = np.random.default_rng([int(seed), 96])
        self.kept, self.answers = None, {}

    topping_up = False

    def draw_B(self):
        return int(self.rng.choice((1, 8))) if self.topping_up else super().draw_B()

    def answer(self, op):
        """the model's answer to a read op that is not emitted yet (the caps on the inputs are conditions on it).  The answer
        to the op that IS emitted next is kept: pinned() hands it to slots(), so that the first run() does not compute it again.
        Asked of a COPY of the model (the arrays are shared: a read replaces them, it never writes into them): the read's flush
        and its auto-compaction must not have happened when a redrawn op is materialised, or a replay of the printed trace,
        which materialises before the read, would see other arguments."""
        import copy
        trial = copy.copy(self.m)
        trial.counts, trial._memo = dict(self.m.counts), {}
        name, args = materialise(self.trace, op, trial)
        want = capture(lambda: getattr(trial, name)(*args))
        self.kept = (op, name, args, want)
        return want

    def emit(self, op):
        if is_read(op) and self.kept is not None and self.kept[0] is op:
            self.answers[len(self.trace["ops"])] = self.kept[1:]
        self.kept = None
        super().emit(op)

    def read(self, kind=None, absent=False):
        if kind is None:                                             # a new kind this mutation has not been followed by yet; the least used one
            after = self.last_mut
            want = [r for r in NEWER_READS if after and (after, r) not in self.pairs]
            least = min(self.used[r] for r in READS12)
            want = [r for r in want if self.used[r] <= least + 2]    # (no kind runs away)
            kind = min(want or READS12, key=lambda r: (self.used[r], READS12.index(r)))
        if kind not in NEWER_READS:
            return super().read(kind, absent)
        return getattr(self, "read_" + kind)(absent=absent) if kind == "best" else getattr(self, "read_" + kind)()

    def mask12(self, none=0.6):
        return self.draw_mask9(self.last_mut == "numbers", none)

    def read_mmr(self, B=None, k=None, m=None, lkey=None, mask=False):
        """B * k * m stays small (the model's selection is a Python loop over the pairs: 12 us each).  A key is redrawn until, with some
        lambda < 1 and k > 1, a query's picks are not the plain top-k."""
        rng = self.rng
        B = B or self.draw_B()
        m = m or int(rng.choice((8, 40, 200)))
        per_query = k is None and rng.random() < 0.2
        if k is None:
            k = int(rng.choice([x for x in (3, 10, 113) if x <= m]))   # (k = 1 cannot move a pick: per-query k holds it)
        while B > 1 and B * k * m > 1600:
            B = {40: 9, 9: 8, 8: 1}[B]
        if B * k * m > 1600 and m < MMR_MAX:
            k = 10
        if per_query and B > 1:
            k = tuple(int(x) for x in rng.choice([x for x in (1, 3, 10) if x <= min(m, k)], B))
        mask = self.mask12() if mask is False else mask
        for attempt in range(2):                                     # (the second with lambda = 0: nothing but the distance between the picks)
            op = ("mmr", B, k, self.k(), m, 0 if attempt == 1 else 1000 + self.k() if lkey is None else lkey, mask)
            got = self.answer(op)
            if "error" in got or got["moved"] or k == 1 or lkey == 4:    # (k = 1 and lambda = 1 cannot move a pick)
                break
        self.emit(op)

    def read_per_group(self, B=None, k=None, g=None, mask=False, deep=False):
        """a key is redrawn until some group has two members or more (g > 1); deep: until a member lies beyond rank 1024"""
        rng = self.rng
        B = B or min(self.draw_B(), 9 if self.m.n_rows() < 5000 else 4)   # (every query is a full ranking of the rows, and a walk over its groups)
        k = k or self.draw_k(B)
        g = g or int(rng.choice((1, 2, 3, 8, 32), p=(0.1, 0.25, 0.35, 0.2, 0.1)))
        mask = self.mask12() if mask is False else mask
        for _ in range(12):
            op = ("per_group", B, k, self.k(), g, mask)
            got = self.answer(op)
            if "error" in got or g == 1 or (got["deep"] >= 1024 if deep else any(len(ids) > 1 for grp in got["groups"] for _, ids, _ in grp)):
                break
        self.emit(op)

    def read_best(self, B=None, k=None, mask=False, absent=False, stage=None):
        """a key is redrawn until at most a quarter of the requests come back empty -- and, with stage, one ends at that stage"""
        rng = self.rng
        B = B or min(self.draw_B(), 8 if self.m.n_rows() < 5000 else 4)   # (every example is a full ranking of the rows in the model)
        if k is None:
            k = tuple(int(x) for x in rng.choice(BEST_KS[:3], B)) if B > 1 and rng.random() < 0.15 else int(rng.choice(BEST_KS, p=(0.15, 0.45, 0.25, 0.15)))
        mask = self.mask12() if mask is False else mask
        for _ in range(12):
            op = ("best", B, k, self.k(), bool(absent), mask)
            got = self.answer(op)
            if "error" in got or (4 * sum(1 for l in got["lists"] if not len(l[0])) <= B and (stage is None or stage in got["bstages"])):
                break
        assert stage is None or "error" in got or stage in got["bstages"], (op, got["bstages"])
        self.emit(op)

    def near(self, n):
        """n rows beside one stored row: the negatives of the next best read's request 0 (best_requests_of)"""
        x = self.live_id()
        for _ in range(n):
            self.emit(("near", self.fresh_ids(1), self.k(), x))

    def copy_of(self, kind):
        """an add, an upsert or a re-add whose vector is a copy of another stored row: the next best read names that row"""
        live = self.m.live_ids()
        x = int(live[int(self.rng.integers(0, live.size))])
        if kind == "add":
            return self.emit(("add", self.fresh_ids(1), self.k(), x))
        i = self.dead_id() if kind == "readd" else None
        if i is None:
            kind, i = "upsert", int(live[(int(np.searchsorted(live, x)) + 1) % live.size])
        self.emit((kind, i, self.k(), x))

    def mix(self, steps, kinds=None):
        kinds = kinds or ("add", "add", "upsert", "upsert", "readd", "remove", "remove", "remove_absent", "bulk", "compact",
                          "compact_shrink", "auto_compact", "codes", "codes", "numbers")
        for _ in range(steps):
            r = self.rng.random()
            if r < 0.1:
                self.toggle()
                continue
            self.turn += 1
            missing = [m for m in kinds if any((m, rd_) not in self.pairs for rd_ in NEWER_READS)]
            kind = missing[self.turn % len(missing)] if missing and r < 0.75 else str(self.rng.choice(kinds))
            self.mutate(kind)
            self.read()
            if self.rng.random() < 0.2:
                self.read()

    def codes_few(self):
        """six codes over every id: above 1024 rows each from about 8000 rows on -- giants under ("set", "pg_cap", 1024)"""
        self.emit(("codes", 0, self.m.id_bound, self.k(), 6))

    def codes_many(self):
        """about two rows per code: the second member of a group lies anywhere in the ranking"""
        self.emit(("codes", 0, self.m.id_bound, self.k(), max(self.groups, self.m.n_live() // 2)))

    def build(self):
        p, rng, e, k = self.p, self.rng, self.emit, self.k
        e(("set", "sparse_filter", int(rng.choice((1, 2)))))
        e(("set", "shadow", 1))
        e(("set", "bounce", 64))
        self.bulk(int(rng.integers(1100, 1400)), p["d"])
        e(("codes", 0, 3000, k(), self.groups))
        self.mutate("numbers")
        # ---- MMR: every stored row a candidate (m = 1024, B = 1); the row written last is candidate 0 of query 0 -- an upsert,
        # then removes and a compaction, each straight in front of an MMR read
        self.read_mmr(B=1, k=3, m=1024, lkey=2, mask=None)
        self.mutate("upsert")
        self.read_mmr(B=4, k=10, m=40, lkey=2, mask=None)
        e(("remove_many", 60, k()))
        e(("compact",))
        self.read_mmr(B=4, k=10, m=40, lkey=1, mask=None)
        # ---- per group: lists under the default cap; the whole column rewritten between two reads; tombstones of wanted codes
        self.mutate("numbers")
        self.read_per_group(B=4, k=10, g=3, mask=None)
        e(("codes", 0, self.m.id_bound, k(), self.groups))
        self.read_per_group(B=4, k=10, g=3, mask=None)
        e(("remove_many", 60, k()))
        self.read_per_group(B=9, k=113, g=3, mask=None)
        # ---- recommend by best: the veto resolves the id written last -- behind a non-monotone add, an upsert and a re-add that
        # copy a stored row (the next read names that row); the scan over tombstones; stage 1 under a mask
        e(("compact",))
        self.mutate("numbers")
        self.read_best(B=4, k=10, mask=None)
        self.copy_of("add")
        self.read_best(B=4, k=10, mask=None)
        self.copy_of("upsert")
        self.read_best(B=4, k=10, mask=None)
        e(("remove_many", 60, k()))
        self.copy_of("readd")
        self.read_best(B=4, k=113, mask=None)
        self.near(1)
        self.read_best(B=4, k=BEST_MAX_K, mask=None, stage=rbd.STAGE_SCAN)   # the 1024 nearest hold fewer than 1024 kept rows: the scan, dead rows in the store
        self.near(2)
        self.read_best(B=4, k=113, mask=("host", k(), 0.5), stage=1)
        # ---- the switches are set here and read mutations later: forced lists, the low cap
        e(("set", "rb_route", 1))
        e(("set", "pg_cap", PG_LOW_CAP))
        for kind in NEWER_READS[:2]:                                 # (ids to re-add are rare later: a compaction forgets them; best had its re-add above)
            self.mutate("readd")
            self.read(kind)
        self.mix(1)
        if p.get("auto"):
            e(("auto_compact", p["auto"]))
            self.read()
        # grow through the doublings (the switches must survive the re-allocations); few codes: giants under the low cap
        for n in (1300, 2500, 4500):
            self.mutate("remove")
            self.bulk(n)
            self.read()
            self.mix(1)
        self.codes_few()
        self.read_per_group(B=4, k=10, g=3, mask=None)                          # giants (above 1024 rows a code): the low cap across the re-allocations
        self.codes_few()                                             # (the same six codes under another key: giants stay giants)
        self.read_best(B=2, k=10, mask=None)                                    # route 1 since the start
        e(("set", "rb_route", 2))
        e(("set", "shadow", 1))
        self.bulk(SMALL_N - 300 - self.m.n_rows())
        self.mutate("add")
        self.read_best(B=2, k=10, mask=None)                                    # route 2 across a re-allocation
        self.read_per_group(B=2, k=10, g=8, mask=("host", k(), 0.9))            # giants under the caller's mask
        e(("set", "rb_route", 0))
        self.bulk(1000)                                              # across SMALL_N upward
        self.mutate("add")
        self.read_mmr(B=1, k=3, m=1024, lkey=3, mask=None)
        self.codes_many()
        e(("set", "pg_cap", 0))
        self.read_per_group(B=4, k=10, g=3, mask=None, deep=True)
        e(("codes", 0, self.m.id_bound, k(), self.groups))          # (back to codes the LUT has numbers for: a numeric mask admits rows again)
        self.read("mmr")
        self.mix(1)
        # back down: most rows go, rows are staged, the compaction takes them along
        e(("auto_compact", 0.0))
        self.read("per_group")
        e(("set", "bounce", 64))
        e(("remove_many", self.m.n_live() - 2600, k()))
        self.read()
        self.mutate("add")
        self.mutate("upsert")
        e(("compact",))
        self.read_mmr(B=4, k=10, m=40, lkey=2, mask=None)
        e(("compact_shrink",))
        self.read("per_group")
        self.mix(1)
        # the row count collides
        e(("compact",))
        self.read()
        n = self.m.n_rows()
        e(("remove_many", 700, k()))
        e(("set", "bounce", 0))
        e(("compact_shrink",))
        self.bulk(n - self.m.n_rows())
        self.read()
        self.read("mmr")
        self.mix(1)
        # auto-compaction inside the read: the ids resolve to the rows AFTER it
        for kind in NEWER_READS:
            e(("auto_compact", p.get("auto") or 0.25))
            e(("remove_many", int(self.m.n_live() * 0.4), k()))
            if kind == "best":
                self.read_best(B=4, k=10, mask=None)
            else:
                self.read(kind)
        if not p.get("auto"):
            e(("auto_compact", 0.0))
        if p["zero"] and self.trace["metric"] == COSINE:
            z = self.fresh_ids(1)
            e(("zero", z))
            for kind in NEWER_READS:
                self.read(kind)
            e(("remove", z))
            self.read()                                              # (answers again; whichever kind is behind -- the top-up counts it)
        if p["misfit"]:
            z = self.fresh_ids(1)
            e(("misfit", z, p["d"] + 3))
            for kind in NEWER_READS:
                self.read(kind)
            e(("remove", z))
            self.read()
        self.read("best", absent=True)
        self.mix(1)
        # everything goes; the refill has another dimension
        e(("remove_many", max(0, self.m.n_live() - 300), k()))
        n = int(rng.integers(1100, 1300))
        e(("codes", 0, self.next_id + n, k(), self.groups))
        e(("reset", n, p["d2"], self.fresh_ids(n), 1, k(), 0.15))
        self.read(NEWER_READS[self.trace["seed"] % 3])              # (the pinned seeds take every new kind here)
        self.read_mmr(B=1, k=3, m=1024, lkey=2, mask=None)
        self.mix(1)
        # what the draws left out -- a third of the pairs per schedule, by its seed: the six pinned ones hold every pair twice over
        for i, (m, r) in enumerate([(m, r) for m in MUTATIONS12 for r in NEWER_READS if m != "reset"]):
            if i % 3 == self.trace["seed"] % 3 and (m, r) not in self.pairs and self.used[r] < 16:   # (at 8 % a kind, a read of the most frequent kind costs eight others)
                self.mutate(m)
                self.read(r)
        # the older cap stays: no read kind below 8 % of the reads (twelve kinds: at most 12 % for the most frequent one).  Here,
        # where the index is smallest, and with the read behind the last bulk counted in
        self.topping_up = True                                       # (batches of 1 and 8 from here on: these reads are there for their count)
        while min(self.used[r] for r in READS12) < 0.08 * (sum(self.used.values()) + 2):
            self.read(min(READS12, key=lambda r: (self.used[r], READS12.index(r))))
        self.bulk(1500)
        self.read()
        return self.trace


LARGE_TWELVE = ("large-twelve", 121, EUCLID, "75 000 rows of d = 64: the searches inside the three composed reads run on the bf16 screening tier, "
                "before and after a compaction and a shrinking compaction refilled to the same row count")


def large_twelve_schedule(seed=LARGE_TWELVE[1], metric=LARGE_TWELVE[2]):
    """at most 40 ops, small batches (in the model every ranking walks 75 000 rows); about two rows per code, so that stage A of
    the search by group completes every query at its depth of 40 -- a deeper stage would leave the screening tier at this size"""
    g = _Gen12(seed, "twelve", metric)
    g.trace["profile"] = "large-twelve"
    e, k = g.emit, g.k

    def reads(deep=False):
        g.read_mmr(B=2, k=10, m=40, lkey=2, mask=None)
        g.read_per_group(B=2, k=10, g=3, mask=None, deep=deep)
        g.read_best(B=2, k=10, mask=None)
    e(("set", "shadow", 1))
    e(("set", "sparse_filter", 1))
    g.bulk(900, 64)
    for n in (30_000, LARGE_ROWS - 30_900):
        g.bulk(n)
        e(("search", 1, 10, k(), None))
    e(("codes", 0, g.m.id_bound, k(), LARGE_ROWS // 2))
    g.mutate("add")
    reads(deep=True)                                                 # (a member beyond rank 1024 of the full ranking)
    g.read_mmr(B=1, k=3, m=1024, lkey=2, mask=None)                  # depth 1024 needs 240 (1024 + 192) rows for the tier: this one is an exact scan
    g.copy_of("upsert")
    reads()
    e(("remove_many", 900, k()))
    e(("compact",))
    reads()
    n = g.m.n_rows()
    e(("remove_many", 900, k()))
    e(("compact_shrink",))
    g.bulk(n - g.m.n_rows())
    reads()
    return g


def schedule(seed, profile, metric=EUCLID):
    """a trace of about 200 ops: see _Gen.build for the phases, PROFILES for what differs between profiles"""
    if profile in ("twelve", "twelve-auto"):
        return _Gen12(seed, profile, metric).build()
    return (_Gen9 if profile in ("nine", "nine-auto") else _Gen)(seed, profile, metric).build()


def pinned(name):
    for n, seed, profile, metric, _ in PINNED:
        if n == name:
            return schedule(seed, profile, metric)
    for n, seed, metric, _ in LARGE_PINNED:
        if n == name:
            return large_schedule(seed, metric)
    for n, seed, profile, metric, _ in NEW_PINNED:
        if n == name:
            return _Gen9(seed, profile, metric).build()
    for n, seed, profile, metric, _ in TWELVE_PINNED + (LARGE_TWELVE[:2] + ("large-twelve",) + LARGE_TWELVE[2:],):
        if n == name:
            g = large_twelve_schedule(seed, metric) if profile == "large-twelve" else _Gen12(seed, profile, metric)
            trace = g.trace if profile == "large-twelve" else g.build()
            if name not in _SLOTS:                                   # the answers the generator had to compute anyway
                _SLOTS[name] = [g.answers.get(step) for step in range(len(trace["ops"]))]
            return trace
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------- store schedules
STORE_PINNED = (
    ("store-euclid-late", 51, EUCLID, dict(table_at="mid", auto=0.0), "device filter switched on mid-life"),
    ("store-cosine-late", 52, COSINE, dict(table_at="mid", auto=0.4), "device filter mid-life, auto-compaction"),
    ("store-dot-early", 53, DOT, dict(table_at="start", auto=0.0), "device filter from the start"),
    ("store-euclid-early", 54, EUCLID, dict(table_at="start", auto=0.4), "device filter from the start, auto-compaction"),
)
NEW_STORE_PINNED = (
    ("store-numeric-early", 55, EUCLID, dict(table_at="start", auto=0.0), "numeric fields, device filter from the start"),
    ("store-numeric-late", 56, COSINE, dict(table_at="mid", auto=0.4), "numeric fields, device filter mid-life, auto-compaction"),
    ("store-numeric-again", 57, DOT, dict(table_at="start", auto=0.0, again=True), "device filter on, off mid-life and on again: the new table takes every number"),
)
TWELVE_STORE_PINNED = (
    ("store-twelve-early", 58, EUCLID, dict(table_at="start", auto=0.0), "MMR, groups and recommend by best through the store, device filter from the start"),
    ("store-twelve-late", 59, COSINE, dict(table_at="mid", auto=0.4), "the same with the device filter switched on mid-life and auto-compaction"),
)
STORE_FILTERS = (("eq", "par", "1"), ("ne", "par", "0"), ("exists", "grp"), ("and", [("exists", "grp"), ("ne", "ver", "2")]),
                 ("or", [("eq", "par", "2"), ("eq", "grp", "g3")]), ("eq", "grp", "g5"))


NUMERIC_STORE_FILTERS = STORE_FILTERS + (
    ("lt", "price", 7.5), ("and", [("ge", "ts", 200000), ("lt", "ts", 700000)]), ("or", [("eq", "grp", "g3"), ("gt", "price", 12.5)]),
    ("gt", "ts", "-inf"), ("le", "price", 3.5))


def store_schedule(seed, metric, table_at="mid", auto=0.0, steps=110, numeric=False, again=False, twelve=False):
    """numeric: the schedules of the numeric fields (doc_fields: ts, price), the filter pool NUMERIC_STORE_FILTERS and the two
    store reads s_recommend and s_with_filters; again: the device filter goes off and on again at two thirds of the life.
    Without them the trace is, draw for draw, the one STORE_PINNED was dealt."""
    rng = np.random.default_rng([int(seed), 98])
    trace = {"seed": int(seed), "profile": "store", "metric": int(metric), "d": 40, "store": True, "groups": 40, "auto": float(auto),
             "table_at": table_at, "ops": []}
    READS_, FILTERS_ = (STORE_READS + NEW_STORE_READS, NUMERIC_STORE_FILTERS) if numeric else (STORE_READS, STORE_FILTERS)
    if numeric:
        trace["numeric"] = True
    if twelve:                                                       # (the schedules of s_mmr, s_groups and s_recommend_best: rows carry duplicates already)
        trace["twelve"] = True
        READS_ = READS_ + NEWER_STORE_READS
    ops = trace["ops"]
    docs, gone, key = set(), set(), [0]

    def k():
        key[0] += 1
        return key[0]

    def flt(none_ok=True):
        return None if none_ok and rng.random() < 0.3 else FILTERS_[int(rng.integers(0, len(FILTERS_)))]

    def read(i):
        kind = READS_[i % len(READS_)]
        kk = int(rng.choice((1, 10, 113)))
        if kind == "s_search":
            ops.append((kind, kk, k()))
        elif kind == "s_with_filter":
            ops.append((kind, max(kk, 10), k(), STORE_FILTERS[int(rng.integers(0, 3))]))   # (a post-filter: unselective ones, or 3 k rows hold no match)
        elif kind == "s_prefiltered":
            B = int(rng.choice(BATCHES))
            ops.append((kind, B, tuple(int(x) for x in rng.choice(KS[:3], B)) if rng.random() < 0.3 else kk, k(), flt(False)))
        elif kind == "s_within":
            ops.append((kind, k(), int(rng.choice((3, 40, 400))), int(rng.choice((8, 256))), flt()))
        elif kind == "s_similar":
            ops.append((kind, int(rng.choice(BATCHES)), kk, k(), flt(), bool(rng.random() < 0.1)))
        elif kind == "s_recommend":
            ops.append((kind, int(rng.choice(BATCHES)), max(kk, 10), k(), flt(), bool(rng.random() < 0.1)))
        elif kind == "s_with_filters":
            B = int(rng.choice(BATCHES))
            ops.append((kind, B, tuple(int(x) for x in rng.choice(KS[:3], B)) if rng.random() < 0.5 else kk, k(), k()))
        elif kind == "s_mmr":
            m = int(rng.choice((8, 40, 200)))
            ops.append((kind, min(max(kk, 3), 10, m), k(), int(rng.integers(0, 4)), m, flt()))
        elif kind == "s_groups":
            ops.append((kind, min(max(kk, 3), 10), k(), int(rng.choice((1, 2, 3, 8), p=(0.1, 0.3, 0.4, 0.2))), flt()))
        elif kind == "s_recommend_best":
            ops.append((kind, int(rng.choice((1, 4, 8))), max(kk, 10), k(), flt(), bool(rng.random() < 0.1)))
        else:
            ops.append((kind, int(rng.choice((1, 8, 9))), kk, k(), flt()))

    if table_at == "start":
        ops.append(("set", "device_filter", 1))
    ops.append(("set", "sparse_filter", int(rng.choice((1, 2)))))
    ops.append(("s_insert_many", 0, 900, k()))
    docs.update(range(900))
    turn = int(seed)
    for step in range(steps):
        if table_at == "mid" and step == steps // 3:
            ops.append(("set", "device_filter", 1))
        if again and step == 2 * steps // 3:                         # off and on again: a new table, every column and LUT sent anew
            ops.append(("set", "device_filter", 0))
            ops.append(("s_insert", 1, k(), -1))
            docs.add(1)
            gone.discard(1)
            ops.append(("set", "device_filter", 1))
            ops.append(("s_prefiltered", 8, 10, k(), ("lt", "price", 7.5)))
        if step == steps // 2:                                       # by construction, whatever the draws bring: a compaction by hand
            ops.append(("s_insert", 0, k(), -1))                     # (an upsert: at least one dead row)
            ops.append(("s_compact",))                               # over the upserts so far, and a by-id read that names an unknown id
            ops.append(("s_similar", 8, 10, k(), None, True))
        r = rng.random()
        live = sorted(docs)
        if r < 0.25:
            ops.append(("s_insert", len(docs) + len(gone) + 1000 + step, k(), -1))
            docs.add(ops[-1][1])
        elif r < 0.55:                                               # an upsert, sometimes of a copy of another version's vector
            ops.append(("s_insert", int(rng.choice(live)), k(), key[0] - 3 if rng.random() < 0.3 and key[0] > 3 else -1))
        elif r < 0.62 and gone:
            j = int(rng.choice(sorted(gone)))
            ops.append(("s_insert", j, k(), -1))
            gone.discard(j)
            docs.add(j)
        elif r < 0.8 and len(live) > 50:
            j = int(rng.choice(live))
            ops.append(("s_delete", j))
            docs.discard(j)
            gone.add(j)
        elif r < 0.85:
            ops.append(("s_delete_absent", 10 ** 7 + step))
        elif r < 0.9:
            ops.append(("s_compact",))
        elif r < 0.95:
            first = max(docs | gone) + 1 if rng.random() < 0.5 else int(rng.choice(live))
            n = int(rng.integers(100, 1300))
            ops.append(("s_insert_many", first, n, k()))
            for j in range(first, first + n):
                docs.add(j)
                gone.discard(j)
        else:
            ops.append(("set", "sparse_filter", int(rng.choice((0, 1, 2)))))
        turn += 1
        read(turn)
        if rng.random() < 0.2:
            turn += 1
            read(turn)
    return trace


def store_pinned(name):
    for n, seed, metric, kw, _ in STORE_PINNED:
        if n == name:
            return store_schedule(seed, metric, **kw)
    for n, seed, metric, kw, _ in NEW_STORE_PINNED:
        if n == name:
            return store_schedule(seed, metric, numeric=True, **kw)
    for n, seed, metric, kw, _ in TWELVE_STORE_PINNED:
        if n == name:
            return store_schedule(seed, metric, numeric=True, twelve=True, **kw)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------- coverage
def read_begins(trace, op, model):
    """What every read does to the model's state, without the oracle: True when the model refuses it (then nothing is uploaded,
    exactly as Model.search & co. raise before they upload), else the staged rows are uploaded and auto-compaction may run."""
    if op[0] in ("grouped", "best") and model.sharded:
        return True
    if (op[5] != "host") if op[0] == "grouped" else (op[0] != "range" and op[-1] is not None and op[-1][0] in ("compiled", "numeric")):
        model.table_uploaded()                                       # (the mask is compiled before the read is called)
    try:
        ids = materialise(trace, op, model)[1][0] if op[0] == "by_id" else None
        if op[0] == "recommend":
            pos, neg = requests_of(trace["seed"], op[3], model, op[1], op[4])
            ids = [i for p, n in zip(pos, neg) for i in p + n]
        if op[0] == "best":
            pos, neg = best_requests_of(trace["seed"], op[3], model, op[1], op[4])
            ids = [i for p, n in zip(pos, neg) for i in p + n]
        model.refusal({"masked": "search", "sparse": "search", "numeric": "search", "recommend": "by_id"}.get(op[0], op[0]), ids)
    except Predicted:
        return True
    model.uploaded()
    return False


def coverage(trace):
    """What a trace reaches, from the trace alone: {"pairs": (mutation, first read after it), "counts": the Log's counters,
    "reads": kinds in order, "errors": how many reads expect an error}.  Error reads are predicted without the oracle."""
    m = Model(trace["metric"])
    pairs, reads, errors, last = set(), [], 0, None
    for op in trace["ops"]:
        if is_read(op):
            reads.append(op[0])
            if last:
                pairs.add((last, op[0]))
                last = None
            errors += read_begins(trace, op, m)
        else:
            apply_mutation(trace, op, m)
            if op[0] in MUTATIONS12 or op[0] == "remove_many":
                last = "remove" if op[0] == "remove_many" else op[0]
    return {"pairs": pairs, "counts": dict(m.counts), "reads": reads, "errors": errors}


_SLOTS = {}


def slots(name, trace):
    """the `expected` list of run() for a pinned trace: computed by the first run, shared by every later one.  For the
    TWELVE_PINNED schedules and large-twelve, pinned() has put the answers in that _Gen12 computed while it built the trace
    (_Gen12.answer / emit: kept by identity of the op it emits next) -- hidden state that ties a trace to its answers by NAME.
    tests/test_lifecycle_cpu.py::test_twelve_traces_are_plain_data_and_replay is the guard: it replays one whole printed trace
    without them and compares name, arguments and answer of every kept slot."""
    return _SLOTS.setdefault(name, [None] * len(trace["ops"]))


# ---------------------------------------------------------------------------------------------------------------- adapters over the engine
class EngineErrors:
    """the engine's exceptions -> the kinds the model predicts"""

    def guarded(self, call):
        v = self.vdb
        try:
            return call()
        except v.VectorNotFound as e:
            raise Predicted("VectorNotFound", e.id)
        except v.DimensionMismatch:
            raise Predicted("DimensionMismatch")
        except v.InvalidVector:
            raise Predicted("InvalidVector")
        except v.VectorDbError as e:
            if "sharded" in str(e):
                raise Predicted("Refused")
            raise
        except ValueError as e:
            if "device filter is off" in str(e):
                raise Predicted("NeedsTable")
            raise


class GpuIndexAdapter(EngineErrors):
    """GpuFlatIndex (devices=None) or one sharded handle (devices=[0, 0, 0]) plus a MetaTable: column 0 holds the group codes,
    the presence bitmap follows add / remove.  Accumulates the engine's own counters over the run (self.seen) and notes the
    route of every plain search (self.route)."""

    def __init__(self, vdb, metric, devices=None):
        self.vdb, self.sharded = vdb, devices is not None
        self.ix = vdb.GpuFlatIndex(vdb.DistanceMetric(metric), keep_host_copy=False, devices=devices)
        self.table = vdb.MetaTable(0)
        self.id_bound = 0
        self.settings = dict(shadow=0, tiers=0, sparse_filter=0, screen=1, large_k=1, sample_cache=1, split=1, split_after=0, pg_cap=0, rb_route=0)
        self.seen = Counter()
        self.route, self.raw = None, None
        self._compactions, self._cap = 0, 0

    def close(self):
        self.table.close()

    # -- mutations
    def _after_write(self):
        st = self.ix.store_stats()
        if st[4] != self._compactions:                               # a compaction ran (by hand or automatic): its chunk counts
            self._compactions = st[4]
            self.seen["compactions"] += 1
            self.seen["chunks_direct"] += st[8]
            self.seen["chunks_bounce"] += st[9]
        if st[2] != self._cap:
            if self._cap and st[2] > self._cap:
                self.seen["grown"] += 1
                self.seen["grown_with_shadow"] += self.settings["shadow"]
            if st[2] and st[2] < self._cap:
                self.seen["shrunk"] += 1
            self._cap = st[2]

    def add(self, id, v):
        self.ix.add(int(id), self.vdb.Vector(v))
        self.table.set_present(int(id), 1, True)
        self.id_bound = max(self.id_bound, int(id) + 1)

    def add_bulk(self, rows, ids):
        ids = np.ascontiguousarray(ids, dtype=U64)
        self.ix.add_bulk(rows, ids=ids)
        lo, hi = int(ids.min()), int(ids.max())
        if hi - lo + 1 == ids.size:
            self.table.set_present(lo, ids.size, True)
        else:
            for i in ids.tolist():
                self.table.set_present(i, 1, True)
        self.id_bound = max(self.id_bound, hi + 1)
        self._after_write()

    def remove(self, ids):
        for i in np.atleast_1d(ids).tolist():
            self.ix.remove(int(i))
            if i < ID_LIMIT:
                self.table.set_present(int(i), 1, False)

    def compact(self, shrink=False):
        got = self.ix.compact(shrink=shrink)
        self._after_write()
        return got

    def set_auto_compact(self, f):
        self.ix.set_auto_compact(f)

    def set_codes(self, first, codes):
        self.table.set_codes(0, int(first), codes)

    def set(self, name, value):
        ix = self.ix
        if self.sharded and name in ("pg_cap", "rb_route"):          # (a sharded handle refuses the two reads and their switches alike)
            self.settings[name] = int(value)
            return
        {"pg_cap": lambda: ix.debug_set_per_group_scan_cap(int(value)), "rb_route": lambda: ix.debug_set_recommend_best_route(int(value)),
         "shadow": lambda: ix.set_shadow(bool(value)), "sample_cache": lambda: ix.set_sample_cache(bool(value)),
         "screen": lambda: ix.set_screen(int(value)), "tiers": lambda: ix.set_tiers(int(value)),
         "sparse_filter": lambda: ix.set_sparse_filter(int(value)), "large_k": lambda: ix.set_large_k(bool(value)),
         "bounce": lambda: ix.debug_set_compact_bounce(int(value)), "split": lambda: ix.set_split(int(value)),
         "split_after": lambda: ix.debug_set_split_after(int(value))}[name]()
        self.settings[name] = int(value)

    def flush(self):
        self.ix.flush()
        self._after_write()

    def layout(self):
        """(layout, conversions so far) of the rows: DESIGN.md 4.3"""
        return self.ix.layout()

    def handed_over(self):
        """did the last search hand a query to the f32 tier or the exact scan (they read f32 rows: a SPLIT store converts back)"""
        st = self.ix.last_stats()
        return bool(st["f32_tier_queries"] or st["exact_queries"])

    # -- reads
    def _masked(self, mask, call):
        """call(**mask keywords) under None | ("host", ok by id) | ("compiled", code): Ne(column 0, code) compiled on the device"""
        if mask is None:
            return call()
        if mask[0] == "host":
            words, bits = dd.id_mask(mask[1])
            return call(id_mask=words, mask_bits=bits)
        cm = self._compile(mask)
        try:
            return call(compiled_mask=cm)
        finally:
            cm.release()

    def _compile(self, mask):
        """("compiled", code): Ne(column 0, code); ("numeric", leaf, const, code): Lt / Le / Gt / Ge(column 0, const), or
        And([Ne(column 0, code), Ge(column 0, const)]) -- one program that reads the code column and the LUT"""
        T, bits = self.table, max(self.id_bound, 1)
        if mask[0] == "compiled":
            return T.compile([(T.NE, 0, int(mask[1]))], bits)
        _, leaf, const, code = mask
        self.seen["numeric_compiles"] += 1
        if leaf == "and":
            return T.compile([(T.NE, 0, int(code)), (T.GE, 0, 0), (T.AND, 0, 0)], bits, consts=[const])
        return T.compile([({"lt": T.LT, "le": T.LE, "gt": T.GT, "ge": T.GE}[leaf], 0, 0)], bits, consts=[const])

    def set_numbers(self, first, values):
        self.table.set_numbers(0, int(first), values)

    def twin(self, model):
        """a fresh index bulk-loaded with the model's survivors and a fresh table with its codes, presence bits and numbers"""
        t = GpuIndexAdapter(self.vdb, model.metric)
        for name in ("pg_cap", "rb_route"):                          # (the twin's counters are compared too: it takes the same routes)
            t.set(name, self.settings[name])
        rows, ids = model.survivors()
        t.add_bulk(rows, ids)
        t.set_codes(0, model.codes[:max(model.col_len, 1)])
        if model.numbers.size:
            t.set_numbers(0, model.numbers)
        return t

    def grouped(self, q, ks, group_of, masks):
        k, kw = (int(ks), {}) if np.isscalar(ks) else (0, {"ks": ks})
        cms = []
        try:
            if masks[0][0] == "host":
                bits = len(masks[0][1])
                kw.update(id_masks=np.stack([dd.id_mask(m[1])[0][:(bits + 63) // 64] for m in masks]), mask_bits=bits)
            else:
                cms = [self._compile(m) for m in masks]
                kw.update(compiled_masks=cms)
            gi, gd, gc = self._read(lambda: self.ix.search_batch_grouped(q, k, group_of, **kw))
        finally:
            for cm in cms:
                cm.release()
        st = self.ix.grouped_stats()
        for j, key in ((2, "grouped_scan"), (3, "grouped_fallback"), (4, "grouped_unfiltered"), (6, "grouped_tiles")):
            self.seen[key] += st[j]
        return {"lists": lists_of(gi, gd, gc), "gstats": st[:6]}

    def recommend(self, pos, neg, ks, mask=None):
        gi, gd, gc = self._read(lambda: self._masked(mask, lambda **kw: self.ix.recommend_batch(pos, neg, ks, **kw)))
        st = self.ix.recommend_stats()
        self.seen["recommend_examples"] += st[1]
        self.seen["recommend_struck"] += st[2]
        return {"lists": lists_of(gi, gd, gc), "rstats": st[1:4]}

    def mmr(self, q, ks, m, lam, mask=None):
        k, kw = (int(ks), {}) if np.isscalar(ks) else (0, {"ks": ks})
        gi, gd, gs, gc = self._read(lambda: self._masked(mask, lambda **mk: self.ix.search_batch_mmr(q, k, int(m), lam, **kw, **mk)))
        out = {"lists": lists_of(gi, gd, gc), "scores": [np.array(gs[b, :int(c)], dtype=F32).view(np.uint32) for b, c in enumerate(gc)]}
        self.seen["bf16_in_mmr"] += self._screened()
        if not self.sharded:                                         # (a sharded handle answers an empty index and keeps no counters)
            st = self.ix.mmr_stats()
            self.seen["mmr_pairs"] += st[3]
            self.seen["mmr_candidates"] += st[2]
            out["mstats"] = st[:5]
        return out

    def per_group(self, q, ks, g, mask=None):
        gi, gd, gcodes, gsizes, gc = self._read(lambda: self._masked(mask, lambda **mk: self.ix.search_batch_per_group(q, ks, int(g), self.table, 0, **mk)))
        groups = [[(int(gcodes[b, j]), np.array(gi[b, j, :int(gsizes[b, j])], dtype=U64), np.array(gd[b, j, :int(gsizes[b, j])], dtype=F32).view(np.uint32))
                   for j in range(int(c))] for b, c in enumerate(gc)]
        out = {"lists": [(np.array([ids[0] for _, ids, _ in grp], dtype=U64), np.array([d[0] for _, _, d in grp], dtype=np.uint32)) for grp in groups],
               "groups": groups}
        self.seen["bf16_in_per_group"] += self._screened()
        if not self.sharded:
            st = self.ix.per_group_stats()
            for j, key in ((2, "per_group_filled"), (3, "per_group_giants"), (5, "per_group_listed")):
                self.seen[key] += st[j]
            out["pstats"] = st[1:7]
        return out

    def best(self, pos, neg, ks, mask=None):
        gi, gd, gn, gc = self._read(lambda: self._masked(mask, lambda **mk: self.ix.recommend_best_batch(pos, neg, ks, **mk)))
        st = self.ix.recommend_best_stats()
        for j, key in ((2, "best_stage0"), (3, "best_stage1"), (4, "best_scan"), (6, "best_list_searches")):
            self.seen[key] += st[j]
        self.seen["bf16_in_best"] += self._screened()
        return {"lists": lists_of(gi, gd, gc), "dn": [np.array(gn[b, :int(c)], dtype=F32).view(np.uint32) for b, c in enumerate(gc)], "bstats": st[:7]}

    def _screened(self):
        """did the last search of the handle run on the bf16 screening tier (the engine's own flag)"""
        return 0 if self.sharded else int(bool(self.ix.last_stats()["bf16_screen"]))

    def _read(self, call):
        try:
            return self.guarded(call)
        finally:
            self._after_write()

    def search(self, q, ks, mask=None):
        self.route = None
        gi, gd, gc = self._read(lambda: self._masked(mask, lambda **kw: self.ix.search_batch_arrays(q, ks, **kw)))
        self.raw = (gi, gd, gc)
        if mask is not None and self.settings["sparse_filter"]:
            sp = self.ix.sparse_stats()
            self.seen["sparse_route"] += sp[0]
            self.route = "sparse" if sp[0] else None
        if self.route is None and not self.sharded:
            st = self.ix.last_stats()
            nq = len(q)
            if st["bf16_screen"]:
                self.route = "bf16"
                self.seen["bf16_shadow_rows"] += st["shadow_rows"]   # the engine's word that the pass read the bf16 shadow
                self.seen["bf16_plain_rows"] += 1 - st["shadow_rows"]
                self.seen["bf16_large_k"] += int(st["kprime"] > 512)
            elif st["exact_queries"] == nq and not st["rows_scanned"] and not st["mfma_queries"] and not st["sample_rows"]:
                small = self.ix.store_stats()[0] <= SMALL_N
                self.route = "direct" if small and nq <= DIRECT_MAX_Q and not self.settings["tiers"] & NO_DIRECT else "exact"
            elif st["exact_queries"] == nq:
                self.route = "exact"
            elif st["rows_scanned"]:
                self.route = "fused"
            else:
                self.route = "dense"
            self.seen["route_" + self.route] += 1
        return {"lists": lists_of(gi, gd, gc)}

    def range(self, q, radii, max_results, mask=None):
        gi, gd, gc, totals = self._read(lambda: self._masked(mask, lambda **kw: self.ix.range_search_batch(q, np.asarray(radii, dtype=F32), max_results, **kw)))
        st = self.ix.range_stats()
        self.seen["range_screened"] += st[0]
        self.seen["range_exact"] += st[1]
        self.seen["range_dense"] += st[2]
        return {"lists": lists_of(gi, gd, gc), "totals": [int(t) for t in totals]}

    def by_id(self, ids, ks, mask=None):
        gi, gd, gc = self._read(lambda: self._masked(mask, lambda **kw: self.ix.search_batch_by_id(ids, ks, **kw)))
        st = self.ix.by_id_stats()
        self.seen["by_id_struck"] += st[1]
        self.seen["by_id_cut"] += st[2]
        return {"lists": lists_of(gi, gd, gc), "struck": st[1], "cut": st[2]}

    def distinct(self, q, ks, mask=None):
        gi, gd, gcodes, gc = self._read(lambda: self._masked(mask, lambda **kw: self.ix.search_batch_distinct(q, ks, self.table, 0, **kw)))
        st = self.ix.distinct_stats()
        for j, key in enumerate(("distinct_a", "distinct_b", "distinct_c")):
            self.seen[key] += st[1 + j]
        return {"lists": lists_of(gi, gd, gc), "codes": [np.array(gcodes[b, :int(c)]) for b, c in enumerate(gc)], "stages": st[1:4]}


def predicted_route(log, settings, op, args):
    """The route a plain, unmasked search with one k is MEANT to take, from the sizes alone (None: not predicted): the direct
    path (at most SMALL_N rows, at most DIRECT_MAX_Q queries), dense scores of a small index, the fused f32 pass above
    SMALL_N, the exact scan for k beyond the tiers' candidate depth."""
    if op[0] != "search" or not np.isscalar(args[1]) or not log.ids.size:
        return None
    n, nq, k = log.n_rows(), len(args[0]), int(args[1])
    if n >= BF16_MIN_ROWS:                                           # the screening tier: k <= 112 always, larger k from 240 (k + 192) rows
        if not settings["screen"]:
            return "fused" if k <= 10 else None
        if k <= 112 or (settings["large_k"] and n >= 240 * (k + 192)):
            return "bf16"
        return "exact"
    if n <= SMALL_N and nq <= DIRECT_MAX_Q and not settings["tiers"] & NO_DIRECT:
        return "direct"
    if k == 300:
        return "exact"
    if k <= 10:
        return "dense" if n <= SMALL_N else "fused"
    return None


class GpuStoreAdapter(EngineErrors):
    """VectorStore over a GpuFlatIndex, driven by the store traces"""

    def __init__(self, vdb, metric, auto_compact=0.0):
        self.vdb = vdb
        self.store = vdb.VectorStore(vdb.DistanceMetric(metric), auto_compact=auto_compact)
        self.seen = Counter()

    def close(self):
        self.store.set_device_filter(False)

    def insert(self, sid, v, fields):
        self.store.insert_with_metadata(sid, self.vdb.Vector(v), self.vdb.Metadata(dict(fields)))

    def delete(self, sid):
        self.guarded(lambda: self.store.delete(sid))

    def compact(self):
        self.store.compact()

    def set(self, name, value):
        if name == "device_filter":
            self.store.set_device_filter(bool(value))
            self.seen["table_switched_on"] += bool(value)
        else:
            self.store.set_sparse_filter(int(value))

    def _out(self, results):
        return [(r.id, int(np.float32(r.distance).view(np.uint32))) for r in results]

    def _note(self):
        ix = self.store.index()
        self.seen["sparse_route"] = ix.sparse_stats()[2]
        self.seen["compactions"] = ix.store_stats()[4]

    def _read(self, call):
        try:
            return self.guarded(call)
        finally:
            self._note()

    def search(self, q, k):
        return self._out(self._read(lambda: self.store.search(self.vdb.Vector(q), k)))

    def search_with_filter(self, q, k, spec):
        return self._out(self._read(lambda: self.store.search_with_filter(self.vdb.Vector(q), k, flt_of(self.vdb, spec))))

    def search_batch_prefiltered(self, q, ks, spec):
        qs = [(self.vdb.Vector(q[b]), k_of(ks, b)) for b in range(len(q))]
        self.seen["prefiltered_compiled" if self.store.device_filter() else "prefiltered_host"] += 1
        self.seen["prefiltered_compiled_on_a_second_table"] += self.store.device_filter() and self.seen["table_switched_on"] >= 2
        return [self._out(r) for r in self._read(lambda: self.store.search_batch_prefiltered(qs, flt_of(self.vdb, spec)))]

    def search_within(self, q, radius, limit, spec):
        return self._out(self._read(lambda: self.store.search_within(self.vdb.Vector(q), radius, limit, flt_of(self.vdb, spec))))

    def search_similar_batch(self, sids, k, spec):
        out = [self._out(r) for r in self._read(lambda: self.store.search_similar_batch(sids, k, flt_of(self.vdb, spec)))]
        st = self.store.index().by_id_stats()
        self.seen["by_id_struck"] += st[1]
        self.seen["by_id_cut"] += st[2]
        return out

    def search_batch_with_filters(self, q, ks, specs):
        qs = [(self.vdb.Vector(q[b]), k_of(ks, b)) for b in range(len(q))]
        out = [self._out(r) for r in self._read(lambda: self.store.search_batch_with_filters(qs, [flt_of(self.vdb, s) for s in specs]))]
        st = self.store.index().grouped_stats()
        self.seen["grouped_scan"] += st[2]
        self.seen["grouped_unfiltered"] += st[4]
        return out

    def recommend_batch(self, requests, k, spec):
        out = [self._out(r) for r in self._read(lambda: self.store.recommend_batch(requests, k, flt_of(self.vdb, spec)))]
        self.seen["recommend_examples"] += self.store.index().recommend_stats()[1]
        return out

    def search_distinct_batch(self, q, k, spec):
        qs = [self.vdb.Vector(x) for x in q]
        out = [self._out(r) for r in self._read(lambda: self.store.search_distinct_batch(qs, k, StoreSim.GROUP_FIELD, flt_of(self.vdb, spec)))]
        self.seen["distinct"] += 1
        return out

    def search_mmr(self, q, k, lam, m, spec):
        out = self._out(self._read(lambda: self.store.search_mmr(self.vdb.Vector(q), k, lam, m, flt_of(self.vdb, spec))))
        self.seen["mmr_pairs"] += self.store.index().mmr_stats()[3] if out else 0
        return out

    def search_groups(self, q, k, g, spec):
        got = self._read(lambda: self.store.search_groups(self.vdb.Vector(q), k, StoreSim.GROUP_FIELD, g, flt_of(self.vdb, spec)))
        out = []
        for value, members in got:
            out.append((f"#{value}", len(members)))
            out.extend(self._out(members))
        if out:
            st = self.store.index().per_group_stats()
            self.seen["per_group_filled"] += st[2]
            self.seen["per_group_groups"] += st[1]
        return out

    def recommend_best_batch(self, requests, k, spec):
        out = [self._out(r) for r in self._read(lambda: self.store.recommend_best_batch(requests, k, flt_of(self.vdb, spec)))]
        st = self.store.index().recommend_best_stats()
        self.seen["best_stage0"] += st[2]
        self.seen["best_later"] += st[3] + st[4]
        return out


# ---------------------------------------------------------------------------------------------------------------- the SPLIT row layout
# after a run of eligible searches an index rewrites its rows in place into their bf16 pieces and low halves; the
# filter pass and the four re-ranks read them as they lie, every other reader (rows_f32) and every mutation (rows_mut) converts
# back first.  A reader that forgets raises nothing.  Three schedules of 75 000 rows with the shadow off (SPLIT_PINNED) interleave
# all nine read kinds with every mutation; LayoutChecked wraps an adapter, follows the rule through every call (LayoutTracker over
# split_schedule.Rule) and compares layout() = (layout, conversions so far) after EVERY step.  SplitRefIndex is the reference
# adapter with that rule inside and three mutants of its own.
from split_schedule import RUN as SPLIT_RUN, Rule as SplitRule, split_hi, split_join, split_lo

LAYOUT_F32, LAYOUT_SPLIT = 0, 1
SPLIT_ROWS = 75_000
PROFILES["split64"] = dict(d=64, d2=64, zero=False, misfit=False)
PROFILES["split40"] = dict(d=40, d2=40, zero=False, misfit=False)
SPLIT_PINNED = (                                                     # name, seed, profile, metric, vdb_flat_set_split at the start, what
    ("split-adaptive-euclid", 91, "split64", EUCLID, 1, "the adaptive rule with a run of 2: every f32 reader and every mutation starts the count again"),
    ("split-mode2-cosine", 92, "split40", COSINE, 2, "d = 40 (a pitch of 64 floats), converted before every eligible search"),
    ("split-off-then-on-dot", 93, "split64", DOT, 0, "mode 0 through all nine read kinds (never converts), then mode 2"),
)
SPLIT_MODES = {0: 0, 1: "adaptive", 2: 2}


def split_schedule(seed, profile, metric, first_mode):
    g = _Gen9(seed, profile, metric)
    e, k, d = g.emit, g.k, g.p["d"]

    def searches(m=SPLIT_RUN + 1):                                   # enough eligible searches in a row for either rule to convert
        for _ in range(m):
            e(("search", 8, 10, k(), None))

    def nine():
        e(("search", 8, 10, k(), None))
        e(("search", 1, 113, k(), None))                             # the large-k re-rank (from 73 200 rows)
        e(("masked", 8, 10, k(), ("host", k(), 0.5)))
        e(("numeric", 8, 10, k(), ("numeric", "ge", k())))
        e(("by_id", 8, 10, k(), False, None))
        e(("recommend", 4, 10, k(), False, None))
        e(("distinct", 4, 10, k(), None))
        e(("grouped", 8, 10, k(), 3, "host", k()))
        e(("range", 4, k(), 40, 256, None))
        e(("set", "sparse_filter", 1))
        e(("sparse", 8, 10, k(), ("host", k(), SPARSE_SHARE)))
        e(("set", "sparse_filter", 0))
    e(("set", "split", first_mode))
    e(("set", "split_after", SPLIT_RUN))
    g.bulk(900, d)
    e(("codes", 0, 80_000, k(), 30))
    e(("numbers", 0, 30, k()))
    for n in (30_000, SPLIT_ROWS - 30_900):                          # growth across re-allocations, across the floor of 65 536 rows
        g.bulk(n)
        e(("search", 1, 10, k(), None))
    if first_mode == 0:
        nine()
        e(("set", "split", 2))
    searches()
    nine()
    # ---- add (staged while the rows are SPLIT under either rule), upsert, remove
    searches()
    e(("add", g.fresh_ids(1), k(), -1))
    searches()
    e(("recommend", 4, 10, k(), False, None))                        # (each of the two straight after a run of searches: over SPLIT rows
    searches()                                                       # under the adaptive rule too)
    e(("by_id", 8, 10, k(), False, None))
    e(("upsert", g.live_id(), k(), -1))
    searches()
    e(("grouped", 8, 10, k(), 3, "host", k()))
    e(("distinct", 4, 10, k(), None))
    e(("remove", g.live_id()))
    searches()
    e(("range", 4, k(), 40, 256, None))
    e(("masked", 8, 10, k(), ("host", k(), 0.5)))
    # ---- compact; a shrinking compaction and a refill to the same row count (which re-allocates)
    e(("remove_many", 200, k()))
    e(("compact",))
    searches()
    nine()
    n = g.m.n_rows()
    e(("remove_many", 900, k()))
    e(("compact_shrink",))
    g.bulk(n - g.m.n_rows())
    searches()
    e(("by_id", 8, 10, k(), False, None))
    e(("numeric", 8, 10, k(), ("numeric", "lt", k())))
    # ---- below 65 536 rows and back
    e(("remove_many", g.m.n_live() - 60_000, k()))
    e(("compact",))
    e(("search", 8, 10, k(), None))
    e(("recommend", 4, 10, k(), False, None))
    g.bulk(SPLIT_ROWS - g.m.n_rows())
    searches()
    # ---- a non-finite row arrives late and is removed: a tombstone still stored -- the conversion walks the rows, not the live bits
    bad = g.fresh_ids(1)
    e(("inf", bad, k()))
    e(("remove", bad))
    searches(SPLIT_RUN + 2)                                          # refused, and not tried again
    e(("grouped", 8, 10, k(), 3, "host", k()))
    e(("compact",))                                                  # the rows change: tried again, and this time it holds
    searches()
    nine()
    searches()
    return g.trace


def split_pinned(name):
    for n, seed, profile, metric, mode, _ in SPLIT_PINNED:
        if n == name:
            return split_schedule(seed, profile, metric, mode)
    raise KeyError(name)


class LayoutTracker:
    """split_schedule.Rule driven by the calls of the adapter interface.  The facts a prediction may take from the read itself
    (certification is data-dependent): whether the last search handed a query to the f32 tier or the exact scan, the stages of a
    distinct read, the counters of a grouped read.  Holds for the schedules above: depths of at most 58 or above 112, fewer than
    262 144 rows (one sample size), the sparse filter 0 or 1, no shadow, no automatic compaction."""

    def __init__(self):
        self.rule = SplitRule("adaptive", 0)
        self.live, self.bad_live, self.settings = set(), set(), dict(split=1, sparse_filter=0)

    def expect(self):
        return self.rule.expect()

    # -- mutations
    def add(self, id, v):
        self.add_bulk(np.asarray(v, dtype=F32)[None, :], [id])

    def add_bulk(self, rows, ids):
        ids = [int(i) for i in np.asarray(ids, dtype=U64)]
        bad = [i for i, r in zip(ids, np.asarray(rows, dtype=F32)) if not np.isfinite(r).all()]
        self.rule.add(len(ids), overwrites=len(self.live.intersection(ids)), bad=bool(bad))
        self.live.update(ids)
        self.bad_live.update(bad)

    def remove(self, ids):
        ids = {int(i) for i in np.atleast_1d(np.asarray(ids, dtype=U64))} & self.live
        if ids:
            self.rule.remove(len(ids))
        self.live -= ids
        self.bad_live -= ids
        assert self.live, "a store emptied by removes starts over: not in these schedules"

    def compact(self, shrink=False):
        self.rule.compact(shrink, bad_left=bool(self.bad_live))

    def set(self, name, value):
        assert name not in ("shadow", "screen", "large_k", "sample_cache") and (name != "sparse_filter" or value in (0, 1)), (name, value)
        self.settings[name] = int(value)
        if name == "split":
            self.rule.mode, self.rule.streak = SPLIT_MODES[int(value)], 0
        if name == "split_after":
            assert int(value) == SPLIT_RUN
            self.rule.streak = 0

    def flush(self):
        self.rule.flush()

    # -- reads
    def _search(self, nq, k, masked, handed_over, by_id=False):
        r = self.rule
        r.flush()
        if by_id:
            r.reader()                                               # the gather / the fold reads the stored rows
        if masked and self.settings["sparse_filter"]:
            return r.reader()                                        # the sparse route: an exact scan of the eligible rows
        assert k <= 58 or k > 112, k
        if k > 112 and r.n >= r.floor and r.n < 240 * (k + 192):
            return r.reader()                                        # large k below its row floor: the exact scan
        r.search(nq, handed_over=handed_over)

    @staticmethod
    def _kmax(ks):
        return int(ks) if np.isscalar(ks) else max(int(x) for x in ks)

    def search(self, got, facts, q, ks, mask=None):
        self._search(len(q), self._kmax(ks), mask is not None, facts["handed_over"])

    def range(self, got, facts, q, radii, max_results, mask=None):
        self.rule.flush()
        self.rule.reader()

    def by_id(self, got, facts, ids, ks, mask=None):
        self._search(len(ids), self._kmax(ks) + 1, mask is not None, facts["handed_over"], by_id=True)

    def recommend(self, got, facts, pos, neg, ks, mask=None):
        m = max(len(p) + len(n) for p, n in zip(pos, neg))
        self._search(len(pos), self._kmax(ks) + m, mask is not None, facts["handed_over"], by_id=True)

    def distinct(self, got, facts, q, ks, mask=None):
        a, b, c = got["stages"]
        # stage A at depth 40; a query it leaves open goes on at depth 1024, which these row counts answer by the exact scan
        self._search(len(q), 40, mask is not None, facts["handed_over"] or a < len(q))

    def grouped(self, got, facts, q, ks, group_of, masks):
        _, _, n_scan, n_over, n_none, _ = got["gstats"]
        assert not n_over
        self.rule.flush()
        if n_scan:
            self.rule.reader()                                       # the grouped scan reads f32 rows
        if n_none:
            self._search(n_none, self._kmax(ks), False, facts["handed_over"])


TRACKED = ("add", "add_bulk", "remove", "compact", "set", "flush")
TRACKED_READS = ("search", "range", "by_id", "recommend", "distinct", "grouped")


class LayoutChecked:
    """An adapter behind a LayoutTracker: every call goes through, and layout() must read what the rule predicts after it."""

    def __init__(self, inner):
        self.inner, self.tracker, self.steps = inner, LayoutTracker(), 0
        self.vdb, self.sharded = getattr(inner, "vdb", None), False

    def __getattr__(self, name):
        call = getattr(self.inner, name)
        if name not in TRACKED + TRACKED_READS:
            return call

        def tracked(*args):
            got = call(*args)
            if name in TRACKED:
                getattr(self.tracker, name)(*args)
            else:
                getattr(self.tracker, name)(got, dict(handed_over=self.inner.handed_over()), *args)
            self.steps += 1
            seen, want = self.inner.layout(), self.tracker.expect()
            if seen != want:
                raise Mismatch(f"layout after {name} (call {self.steps}): {seen}, predicted {want}; rule {vars(self.tracker.rule)}")
            return got
        return tracked


def garble_as_split_bytes(v, ld):
    """a row's SPLIT bytes taken as ld floats: what a reader sees that forgets rows_f32()"""
    bits = np.zeros(ld, dtype=np.uint32)
    bits[:v.size] = np.asarray(v, dtype=F32).view(np.uint32)
    return np.concatenate([split_hi(bits), split_lo(bits)]).view(np.uint32).view(F32)[:v.size].copy()


def garble_as_joined_f32(v, ld):
    """an f32 row written into SPLIT rows and then "converted back": its words joined as if they were the two planes"""
    row = np.zeros(ld, dtype=F32)
    row[:v.size] = v
    w = row.view(np.uint16)
    return split_join(w[:ld], w[ld:]).view(F32)[:v.size].copy()


SPLIT_MUTANTS = ("gather_takes_bytes", "fold_takes_bytes", "append_into_split", "refusal_forgotten")


class SplitRefIndex(RefIndex):
    """The reference adapter with the layout rule inside (a LayoutTracker of its own: layout() is what the engine's would be).
    mutant: the by-id gather / every example of a recommend fold but the first reads the bytes as they lie while the rows are SPLIT;
    an append is written into SPLIT rows and the store then converted back; a refusal is forgotten after a search."""

    def __init__(self, metric, mutant=None):
        super().__init__(metric)
        assert mutant in (None,) + SPLIT_MUTANTS
        self.mutant, self.own, self.split_at_read, self.reading = mutant, LayoutTracker(), False, None

    def layout(self):
        return self.own.expect()

    def handed_over(self):
        return False

    def knn(self, rows, ids, q, k):
        try:
            return super().knn(rows, ids, q, k)
        except oracle.OracleError:                                   # (bytes taken as floats may hold a NaN: the engine would fail the search)
            raise Predicted("NanDistance")

    @property
    def ld(self):
        return (self.d + 31) // 32 * 32

    def stored(self, rows, first):
        if self.mutant == "append_into_split" and self.own.rule.layout == LAYOUT_SPLIT:
            return np.stack([garble_as_joined_f32(r, (rows.shape[1] + 31) // 32 * 32) for r in rows])
        return rows

    def uploaded(self):
        super().uploaded()
        self.own.rule.flush()
        self.split_at_read = self.own.rule.layout == LAYOUT_SPLIT     # what a gather that does not convert back would find

    def example_of(self, id, position):
        v = self.vector_of(id)
        takes = (self.mutant == "gather_takes_bytes" and self.reading == "by_id") or \
                (self.mutant == "fold_takes_bytes" and self.reading == "recommend" and position)
        return garble_as_split_bytes(v, self.ld) if takes and self.split_at_read else v

    def by_id(self, ids, ks, mask=None):
        self.reading = "by_id"
        if self.mutant != "gather_takes_bytes":
            return self._read("by_id", ids, ks, mask)
        ids = np.asarray(ids, dtype=U64)                             # RefIndex.by_id with the gather through example_of
        self.refusal("by_id", ids)
        self.uploaded()
        rows, bids = self.block(mask)
        out, struck, cut = [], 0, 0
        for b, own in enumerate(ids):
            kb = k_of(ks, b)
            oi, od = self.knn(rows, bids, self.example_of(own, 0), kb + 1)
            oi, od, hit, _cut = bd.strike(oi, od, own, kb)
            struck, cut = struck + bool(hit), cut + bool(_cut)
            out.append((oi, od.view(np.uint32)))
        got = {"lists": out, "struck": struck, "cut": cut} if np.isscalar(ks) else {"lists": out}
        self.own.by_id(got, dict(handed_over=False), ids, ks, mask)
        return got

    def _read(self, name, *args):
        self.reading = name
        got = getattr(RefIndex, name)(self, *args)
        if name == "distinct":                                       # (the reference adapter names no stages: every query ends in stage A here or not)
            got = dict(got, stages=self.model_stages(*args))
        getattr(self.own, name)(got, dict(handed_over=False), *args)
        if self.mutant == "refusal_forgotten":
            self.own.rule.refused = False
        return got

    def model_stages(self, q, ks, mask=None):
        rows, ids = self.block(mask)
        a = 0
        for b in range(len(q)):
            rank = self.knn(rows, ids, q[b], len(rows))
            a += dd.stage_of(rank, self.codes_seen(), k_of(ks, b), self.n_live()) == "A"
        return [a, len(q) - a, 0]

    def search(self, *a):
        return self._read("search", *a)

    def range(self, *a):
        return self._read("range", *a)

    def distinct(self, *a):
        return self._read("distinct", *a)

    def grouped(self, *a):
        return self._read("grouped", *a)

    def recommend(self, *a):
        return self._read("recommend", *a)

    # -- mutations
    def add(self, id, v):
        super().add(id, v)
        self.own.add(id, v)

    def add_bulk(self, rows, ids):
        super().add_bulk(rows, ids)
        self.own.add_bulk(rows, ids)

    def remove(self, ids):
        super().remove(ids)
        self.own.remove(ids)

    def compact(self, shrink=False):
        out = super().compact(shrink)
        self.own.compact(shrink)
        return out

    def set(self, name, value):
        self.own.set(name, value)

    def flush(self):
        super().flush()
        self.own.flush()

"""Stateful lifecycle tests of the HNSW index and its device mirror: a model, a reference adapter with mutants, a schedule
generator and a runner (no GPU, no import of the product).  Conventions of tests/lifecycle.py.

A TRACE is plain data: {"seed", "metric", "d", "m", "efc", "ops": [tuple, ...]}.  Every vector, mask and query is derived from
(trace seed, the key an op carries) and every id and level stands in the op itself, so a trace can be printed, pasted into a test
as a literal and replayed with run(trace, adapter).  run() applies every op to the adapter and to the MODEL and compares after
every read: ids, order, counts and distance BITS, the whole graph, vector bits, or the error the model predicts.  There is no
tolerance anywhere.

MUTATIONS (op[0] is the kind the pair table counts; what an op does follows from its fields alone)
  ("add", id, key) / ("add_level", id, key, level) / ("jump", id, key)                     a fresh id: drawn level / forced level / far beyond cap_ids
  ("readd_present" | "readd_removed" | "readd_entry", id, key, level)                      level -1 = drawn
  ("remove" | "remove_absent" | "remove_entry", id)
  ("bulk", key, n, first, repl)           ids first .. first + n - 1, position p replaced by id i for every (p, i) of repl
  ("set_build", frontier_only) / ("set_traversal", host_only) / ("set_filter_scan", limit)
READS
  ("search", qkey, B, k, ef, near)
  ("masked" | "filtered", qkey, B, k, ef, near, mkey, selectivity, bits_mode)              host id mask / compiled from a code column;
                                          mask_bits = node ids + (-7, 0, 37)[bits_mode], so it cuts or covers the newest ids
  ("scan", qkey, B, k, ef, near, mkey, over, api)   a mask of (filter-scan limit + over) present nodes, half of them the newest
  ("graph",)  ("get_vector", id)
  qkey ZERO_QUERY = an all-zero query (InvalidVector under Cosine on every route); near = (key, n, i): query 0 IS row i of the
  block of n vectors of that key -- the vector a mutation just stored; i may be a tuple of rows, for the first queries.
Every walk read is made twice, route "device" then route "host" (vdb_hnsw_set_traversal): both must give the model's answer.

THE MODEL (Model): graph, len, entry point and the plain search are oracle.HnswOracle's (same seed, same insertion order); masked
and filtered walks are hnsw_filter_restatement.Walker over the oracle's graph and the model's current vector per id; the filter
scan is oracle.flat_search over the present eligible nodes.

THE MIRROR'S BOOKKEEPING is restated in one place, MirrorBook: the growth rule cap = n + n / GROW_DIV + GROW_PAD (for node ids
and for pooled upper lists), the causes of a full rebuild (a mutation set mirror_full / an id beyond cap_ids / the pool beyond
cap_upper, first cause wins, the bulk path's own check with its reserve included), the pool's hand-out of upper-list slots and
the dirty-node rule (Log.dirty_of: the new node and every owner of a back-link).  Log.fresh_run restates where a bulk build
syncs: before its first block and before the replay of every block but the last, never after the last.  From this the model
predicts ALL EIGHT counters of vdb_hnsw_mirror_stats exactly, after every read -- [4] and [5] inside a bulk too, because the
per-block syncs are sequenced by the host and the dirty set of every insert follows from the graph.  No counter is only monotonic.

THE REFERENCE ADAPTER (MirrorRef) answers by another path: a second oracle, and a SNAPSHOT of its graph updated by the product's
rule -- per id the vector version the mirror's row stands for, the level, the layer-0 list and a slot in a pool of upper lists,
every list entry carrying the version of the neighbour's vector as of the copy (nbr0_row / nbrU_row).  A remove, a re-add or a
capacity overflow copies the whole graph, otherwise only the dirty nodes are copied.  Device-route walks are Walker over the
snapshot, host-route walks Walker over the second oracle.  Its MUTANTS carry one stale-state defect each, modelled on a field of
Graph (vdb_hnsw.cpp); tests/test_hnsw_lifecycle_cpu.py requires the pinned schedules to catch every one."""
import numpy as np

import oracle
from hnsw_filter_restatement import Walker
from lifecycle import Mismatch, Predicted, capture, diff, rng_of

F32, U64 = np.float32, np.uint64
EUCLID, COSINE, DOT = 0, 1, 2
GROW_DIV, GROW_PAD = 4, 1024           # sync_mirror: capacity of a rebuild = n + n / 4 + 1024
BLOCK, SPEC_MIN = 64, 32               # build_speculative: inserts per block (WALKS); shortest run that is built that way
SCAN_MAX_K, SCAN_CAP = 2048, 131072
MAX_LEVEL = 15
ZERO_QUERY = -2
KEY_BITS = 40                          # a snapshot key = id | (version of the id's vector << KEY_BITS)
KEY_MASK = (1 << KEY_BITS) - 1
MUTATIONS = ("add", "add_level", "readd_present", "readd_removed", "readd_entry", "remove", "remove_absent", "remove_entry",
             "bulk", "jump", "set_build", "set_traversal", "set_filter_scan")
READS = ("search", "masked", "filtered", "scan", "graph", "get_vector")
BULK_SIZES = (1, 31, 32, 33, 64, 65, 130)
SELECTIVITIES = (1.0, 0.5, 0.1, 0.0)
BITS_MODES = (-7, 0, 37)
STAT_NAMES = ("rebuilds", "rebuilds_mutation", "rebuilds_id_capacity", "rebuilds_upper_capacity", "scatters", "scattered_nodes",
              "cap_ids", "cap_upper")


# ---------------------------------------------------------------------------------------------------------------- derived data
def block_of(seed, key, n, d):
    return rng_of(seed, key).standard_normal((n, d)).astype(F32)


def queries_of(trace, qkey, B, near):
    d = trace["d"]
    q = np.zeros((B, d), dtype=F32) if qkey == ZERO_QUERY else rng_of(trace["seed"], qkey, 1).standard_normal((B, d)).astype(F32)
    if near is not None and qkey != ZERO_QUERY:
        key, n, i = near
        rows = block_of(trace["seed"], key, n, d)[list(i) if isinstance(i, tuple) else [i]]
        q[:len(rows)] = rows[:B]
    return q


def bulk_ids(op):
    _, _, n, first, repl = op
    ids = list(range(first, first + n))
    for p, i in repl:
        ids[p] = i
    return ids


def splitmix_unit(state):
    z = state
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & 0xffffffffffffffff
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & 0xffffffffffffffff
    z ^= z >> 31
    return (z >> 11) * (1.0 / 9007199254740992.0)


# ---------------------------------------------------------------------------------------------------------------- the mirror's bookkeeping
class MirrorBook:
    """sync_mirror's decisions without its arrays.  `g` (every sync) answers n_ids, is_present(id), level(id), present_ids()."""

    def __init__(self):
        self.exists, self.full, self.cause = False, True, 1
        self.cap_ids = self.cap_upper = self.used = self.mirror_ids = 0
        self.up_off = {}                                             # id -> first slot of its upper lists (h_up_off)
        self.dirty, self.dirty_set = [], set()
        self.c = [0] * 6

    def id_overflows(self, n):
        return n > self.cap_ids

    def pool_overflows(self, need):
        return self.used + need > self.cap_upper

    def mark(self, ids):
        for i in ids:
            if i not in self.dirty_set:
                self.dirty_set.add(i)
                self.dirty.append(i)

    def force_full(self):                                            # a remove, a re-add
        self.full, self.cause = True, 1

    def reserve(self, max_id, up_total):                             # the bulk path's own capacity check
        if not self.full and self.exists and (max_id + 1 > self.cap_ids or up_total > self.cap_upper):
            self.cause = 2 if max_id + 1 > self.cap_ids else 3
            self.full = True

    def stats(self):
        return self.c + [self.cap_ids, self.cap_upper]

    def sync(self, g, reserve_ids=0, reserve_upper=0):
        """-> None (nothing to do), ("scatter", ids) or ("full", cause)"""
        n = g.n_ids
        if self.full or not self.exists:
            cause = self.cause if self.exists else 1
        else:
            cause = 2 if self.id_overflows(n) else 0
        if not cause:
            for i in self.dirty:
                if not g.is_present(i) or g.level(i) == 0 or i in self.up_off:
                    continue
                if self.pool_overflows(g.level(i)):
                    cause = 3
                    break
                self.up_off[i] = self.used
                self.used += g.level(i)
        if not cause:
            if not self.dirty:
                return None
            ids = self.dirty
            self.c[4] += 1
            self.c[5] += len(ids)
            self.dirty, self.dirty_set = [], set()
            self.mirror_ids = n
            return ("scatter", ids)
        present = g.present_ids()
        n_upper = sum(g.level(i) for i in present)
        self.cap_ids = max(n + n // GROW_DIV + GROW_PAD, reserve_ids, 1)
        self.cap_upper = max(n_upper + n_upper // GROW_DIV + GROW_PAD, reserve_upper, 1)
        self.up_off, off = {}, 0
        for i in present:
            if g.level(i):
                self.up_off[i] = off
            off += g.level(i)
        self.used = off
        self.c[0] += 1
        self.c[cause] += 1
        self.exists, self.full, self.cause, self.mirror_ids = True, False, 1, n
        self.dirty, self.dirty_set = [], set()
        return ("full", cause)


# ---------------------------------------------------------------------------------------------------------------- graph + bookkeeping
class Log:
    """What the model and the reference adapter share: an oracle graph driven in the product's insertion order, the current
    vector per id, the three settings, and the MirrorBook told about every mutation the way vdb_hnsw.cpp tells its mirror."""
    book_class = MirrorBook

    def __init__(self, trace):
        self.metric, self.d, self.m, self.efc, self.seed = (int(trace[k]) for k in ("metric", "d", "m", "efc", "seed"))
        self.o = oracle.HnswOracle(self.metric, m=self.m, ef_construction=self.efc, ef_search=50, seed=self.seed)
        self.vec, self.lvl, self.ver, self.order = {}, {}, {}, {}
        self.removed = set()
        self.n_ids = self.seq = self.sum_levels = self.draws = 0
        self.frontier, self.host_only, self.filter_scan = True, False, 0
        self.book = self.book_class()
        self.routes = []                                             # of every walk read, in order: "walk" | "scan" | "empty"

    # -- the graph view MirrorBook.sync reads
    def is_present(self, i):
        return i in self.vec

    def level(self, i):
        return self.lvl[i]

    def present_ids(self):
        return sorted(self.vec)

    def seen(self, i):
        return i in self.vec or i in self.removed

    # -- levels ahead of the inserts (add_fresh_rows draws a whole run's levels before its first insert)
    def peek_levels(self, n):
        out = []
        for t in range(1, n + 1):
            state = (self.seed + (self.draws + t) * 0x9e3779b97f4a7c15) & 0xffffffffffffffff
            out.append(oracle.hnsw_level_from_unit(splitmix_unit(state), self.m, MAX_LEVEL + 1))
        return out

    def dirty_of(self, i):
        """mark_dirty: the new node, and every node that got a back-link (present, and it has the layer)"""
        out = [i]
        for l in range(self.lvl[i] + 1):
            for x in self.o.neighbors(i, l) or []:
                if x in self.vec and self.lvl[x] >= l and x not in out:
                    out.append(x)
        return out

    def on_readd(self, i):
        self.book.force_full()

    def on_remove(self, i):
        self.book.force_full()

    def on_insert(self, i, old):
        pass

    def on_sync(self, what):
        pass

    def _insert(self, i, v, level):
        readd, old = self.seen(i), self.vec.get(i)
        if i in self.vec:
            self.sum_levels -= self.lvl[i]
        want = self.peek_levels(1)[0] if level < 0 else None
        self.o.insert(i, v, level)
        if level < 0:
            self.draws += 1
            assert self.o.level(i) == want, "the level stream was restated wrongly"
        self.lvl[i] = self.o.level(i)
        self.sum_levels += self.lvl[i]
        self.vec[i] = np.array(v, dtype=F32)
        self.removed.discard(i)
        self.n_ids = max(self.n_ids, i + 1)
        self.ver[i] = self.ver.get(i, 0) + 1
        self.order[i] = self.seq
        self.seq += 1
        self.on_insert(i, old)
        if readd:
            self.on_readd(i)
        self.book.mark(self.dirty_of(i))

    # -- mutations, as the adapters spell them
    def add(self, i, v, level=-1):
        self._insert(int(i), v, int(level))

    def remove(self, i):
        i = int(i)
        if i not in self.vec:
            return
        self.o.remove(i)
        self.sum_levels -= self.lvl[i]
        del self.vec[i]
        self.removed.add(i)
        self.on_remove(i)

    def set(self, name, value):
        if name == "build":
            self.frontier = bool(value)
        elif name == "traversal":
            self.host_only = bool(value)
        else:
            self.set_filter_scan(int(value))

    def set_filter_scan(self, limit):
        self.filter_scan = limit

    def bulk(self, ids, rows):
        """add_rows: the batch is split at every id seen before and at the second occurrence of an id"""
        ids = [int(i) for i in ids]
        run, in_run = [], set()
        for t, i in enumerate(ids):
            if not self.seen(i) and i not in in_run:
                run.append(t)
                in_run.add(i)
                continue
            self.fresh_run([ids[j] for j in run], [rows[j] for j in run])
            run, in_run = [], set()
            self._insert(i, rows[t], -1)
        self.fresh_run([ids[j] for j in run], [rows[j] for j in run])

    def after_last_block(self, ids):
        pass

    def fresh_run(self, ids, rows):
        """add_fresh_rows: a run of ids never seen, each once"""
        n = len(ids)
        if n == 0:
            return
        if not (self.frontier and not self.host_only and n >= SPEC_MIN):
            for i, v in zip(ids, rows):                              # the row-scan build: no sync
                self._insert(i, v, -1)
            return
        max_id, up_total = max(ids), self.sum_levels + sum(self.peek_levels(n))
        self.book.reserve(max_id, up_total)
        self.on_sync(self.book.sync(self, max_id + 1, up_total))
        blocks = [list(range(c, min(c + BLOCK, n))) for c in range(0, n, BLOCK)]
        for b, blk in enumerate(blocks):
            if b + 1 < len(blocks):
                self.on_sync(self.book.sync(self, max_id + 1, up_total))
            for t in blk:
                self._insert(ids[t], rows[t], -1)
        assert self.sum_levels == up_total, "the levels of the run were peeked wrongly"
        self.after_last_block([ids[t] for t in blocks[-1]])

    def read_sync(self):
        self.on_sync(self.book.sync(self))

    # -- which route a walk read takes, with the sync that comes with it
    def eligible_present(self, elig):
        return [i for i in sorted(self.vec) if i < elig.size and elig[i]]

    def scan_limit(self):
        return self.filter_scan

    def route(self, api, k, elig, route):
        """-> "walk" | "scan" | "empty"; brings the mirror up to date where the product does"""
        if not self.vec:
            return "empty"
        if api == "filtered":
            self.read_sync()                                         # present_mask_device, before the route is known
        if elig is not None:
            ok = self.eligible_present(elig)
            if not ok:
                return "empty"
            limit = self.scan_limit()
            if limit and 0 < k <= SCAN_MAX_K and len(ok) <= min(limit, SCAN_CAP):
                return "scan"
        return "walk"

    def advance_read(self, api, k, elig, route):
        """one pass of a walk read, without its answer: route it, note the route of the device pass, sync the mirror where the
        product does (a filtered read has done so in route(); a host pass, a scan and an empty mask never do)"""
        r = self.route(api, k, elig, route)
        if route == "device":
            self.routes.append(r)
            if r == "walk" and api != "filtered":
                self.read_sync()
        return r

    def zero_refused(self, q):
        return self.metric == COSINE and bool((np.abs(q).sum(axis=1) == 0).any())

    def graph(self):
        ep = self.o.entry_point()
        lists = {i: [self.o.neighbors(i, l) for l in range(self.lvl[i] + 1)] for i in sorted(self.vec)}
        return {"graph": (len(self.o), ep, {i: self.lvl[i] for i in sorted(self.vec)}, lists)}

    def get_vector(self, i):
        if i not in self.vec:
            raise Predicted("VectorNotFound")
        return {"vector": self.vec[i].view(np.uint32).copy()}

    def mirror_stats(self):
        return self.book.stats()


def answer_of(per_query):
    return {"lists": [(np.asarray(i, dtype=U64), np.asarray(d, dtype=F32).view(np.uint32)) for i, d in per_query]}


class Model(Log):
    def walk(self, api, q, k, ef, elig, route):
        r = self.advance_read(api, k, elig, route)
        if self.vec and self.zero_refused(q):
            raise Predicted("InvalidVector")
        if r == "empty":
            return answer_of([((), ())] * len(q))
        try:
            if r == "scan":
                ids = np.array(self.eligible_present(elig), dtype=U64)
                rows = np.stack([self.vec[int(i)] for i in ids])
                return answer_of([oracle.flat_search(self.metric, rows, qb, k, ids=ids) for qb in q])
            if elig is None:
                return answer_of([self.o.search(qb, k, ef) for qb in q])
            w = Walker(self.o, self.metric, self.vec)
            return answer_of([w.search(qb, k, ef, eligible=lambda i: i < elig.size and bool(elig[i])) for qb in q])
        except oracle.OracleError as e:
            raise Predicted("InvalidVector" if e.code == oracle.ERR_INVALID_VECTOR else f"oracle {e.code}")


# ---------------------------------------------------------------------------------------------------------------- the reference adapter
class _Snapshot:
    """the graph Walker walks on the device route: the mirror's arrays, as dictionaries"""

    def __init__(self, ref):
        self.ref = ref

    def entry_point(self):
        ep, top = self.ref.o.entry_point()                           # (the entry point and max_level are launch parameters, not mirrored)
        rec = self.ref.rec.get(ep)
        if ep is None or rec is None:
            return None, 0
        return ep | (rec["ver"] << KEY_BITS), top

    def neighbors(self, key, layer):
        rec = self.ref.rec.get(key & KEY_MASK)
        if rec is None:
            return []
        if layer == 0:
            return rec["l0"]
        return self.ref.pool.get(rec["off"] + layer - 1, []) if layer <= rec["level"] else []


class MirrorRef(Log):
    clamp_before_sync = False

    def __init__(self, trace):
        super().__init__(trace)
        self.rec, self.pool = {}, {}
        self.rows_by_key = {}                                        # every vector an id ever had: what a cached row may still lead to
        self.dead = {}                                               # id -> vectors it had before a re-add (rows the inner flat handle keeps)

    def on_insert(self, i, old):
        self.rows_by_key[i | (self.ver[i] << KEY_BITS)] = self.vec[i]
        if old is not None:
            self.dead.setdefault(i, []).append(old)

    def key_list(self, ids):
        return [x | (self.ver[x] << KEY_BITS) for x in ids if x in self.vec]      # (an absent neighbour has no row: never expanded)

    def copy_node(self, i):
        if i >= self.book.cap_ids:                                   # outside the id arrays: sync_mirror's guard refuses the scatter
            raise Predicted("DeviceError")                           # (unreachable under the real rule)
        if i not in self.vec:
            self.rec.pop(i, None)
            return
        lvl, off = self.lvl[i], self.book.up_off.get(i, 0)
        if lvl and off + lvl > self.book.cap_upper:                  # a list past the pool: refused by the same guard
            raise Predicted("DeviceError")
        self.rec[i] = {"ver": self.ver[i], "level": lvl, "off": off, "l0": self.key_list(self.o.neighbors(i, 0) or [])}
        for l in range(1, lvl + 1):
            self.pool[off + l - 1] = self.key_list(self.o.neighbors(i, l) or [])

    def copy_all(self, cause):
        self.rec, self.pool = {}, {}
        for i in sorted(self.vec):
            self.copy_node(i)

    def on_sync(self, what):
        if what is None:
            return
        if what[0] == "full":
            self.copy_all(what[1])
        else:
            for i in what[1]:
                self.copy_node(i)

    def scan(self, q, k, elig):
        out = []
        for qb in q:
            cand = []
            for i in self.eligible_present(elig):
                for v in self.scan_rows(i):
                    cand.append((oracle.distance(self.metric, qb, v), i))
            cand.sort(key=lambda t: (t[0], t[1]))
            out.append(([i for _, i in cand[:k]], [d for d, _ in cand[:k]]))
        return answer_of(out)

    def scan_rows(self, i):
        return [self.vec[i]]

    def walk(self, api, q, k, ef, elig, route):
        clamp = self.book.mirror_ids
        r = self.route(api, k, elig, route)
        if r == "walk" and route == "device":
            self.read_sync()
        if self.vec and self.zero_refused(q):
            raise Predicted("InvalidVector")
        if r == "empty":
            return answer_of([((), ())] * len(q))
        if r == "scan":
            return self.scan(q, k, elig)
        if route == "host":
            w, bits = Walker(self.o, self.metric, self.vec), None if elig is None else elig.size
        else:
            w = Walker(_Snapshot(self), self.metric, self.rows_by_key)
            bits = None if elig is None else min(elig.size, clamp if self.clamp_before_sync else self.book.mirror_ids)
        ok = None if elig is None else (lambda key: (key & KEY_MASK) < bits and bool(elig[key & KEY_MASK]))
        out = []
        for qb in q:
            ids, ds = w.search(qb, k, ef, eligible=ok)
            out.append(([int(x) & KEY_MASK for x in ids], ds))
        return answer_of(out)


# ---- the mutants: one stale-state defect each
class BackLinksNotDirty(MirrorRef):
    """mark_dirty is not called for the owners of the back-links: the scatter carries only the new node"""

    def dirty_of(self, i):
        return [i]


class ReaddKeepsNeighbourRows(MirrorRef):
    """readd_row does not set mirror_full: lists that name the id keep its old device row (nbr0_row / nbrU_row)"""

    def on_readd(self, i):
        self.book.up_off.pop(i, None)


class ReaddKeepsUpperSlot(MirrorRef):
    """readd_row neither rebuilds nor resets h_up_off[id]: at a higher level the node's lists spill into the next node's slots
    (every list that names the id is refreshed, so only the slot is stale)"""

    def on_readd(self, i):
        for x in sorted(self.vec):
            if any(i in (self.o.neighbors(x, l) or []) for l in range(self.lvl[x] + 1)):
                self.book.mark([x])


class RemoveLeavesMirror(MirrorRef):
    """vdb_hnsw_remove does not set mirror_full: the node stays in d_row_of and in every list that named it"""

    def on_remove(self, i):
        pass


class _BookIdOffByOne(MirrorBook):
    def id_overflows(self, n):
        return n > self.cap_ids + 1


class IdCapacityOffByOne(MirrorRef):
    """n > cap_ids is tested one too late: the id equal to cap_ids goes to the scatter, outside the id arrays -- the read that
    needed it is lost to sync_mirror's guard"""
    book_class = _BookIdOffByOne


class _BookPoolOffByOne(MirrorBook):
    def pool_overflows(self, need):
        return self.used + need > self.cap_upper + 1


class UpperPoolOffByOne(MirrorRef):
    """n_upper_used + level > cap_upper is tested one too late: the node whose lists end one slot past the pool goes to the scatter"""
    book_class = _BookPoolOffByOne


class RebuildDropsPooledLists(MirrorRef):
    """a capacity rebuild reads h_up_off as of the last rebuild: nodes that got their slot from the pool since have no upper lists"""

    def __init__(self, trace):
        super().__init__(trace)
        self.pooled = set()

    def on_sync(self, what):
        if what is not None and what[0] == "scatter":
            self.pooled.update(i for i in what[1] if self.lvl.get(i))
        super().on_sync(what)

    def copy_all(self, cause):
        super().copy_all(cause)
        if cause in (2, 3):
            for i in self.pooled & set(self.rec):
                for l in range(1, self.rec[i]["level"] + 1):
                    self.pool[self.rec[i]["off"] + l - 1] = []
        self.pooled = set()


class LastChunkNotSynced(MirrorRef):
    """the dirty nodes of a bulk's last, partial block miss the next sync and reach the mirror one read late"""

    def __init__(self, trace):
        super().__init__(trace)
        self.late = []

    def after_last_block(self, ids):
        if len(ids) % BLOCK and not self.book.full:
            self.late, self.book.dirty, self.book.dirty_set = self.book.dirty, [], set()

    def read_sync(self):
        late, self.late = self.late, []
        super().read_sync()
        self.book.mark(late)


class MaskClampedToOldIds(MirrorRef):
    """a masked walk clamps mask_bits to mirror_ids BEFORE upload_mirror: ids added since the last sync are never eligible"""
    clamp_before_sync = True


class ScanSeesReplacedRow(MirrorRef):
    """the filter scan does not AND the graph's view in: the dead row of a re-added id is scanned too"""

    def scan_rows(self, i):
        return [self.vec[i]] + self.dead.get(i, [])


class ToggleKeepsRoute(MirrorRef):
    """vdb_hnsw_set_filter_scan(0) takes effect one routed read late"""

    def __init__(self, trace):
        super().__init__(trace)
        self.lingering = 0

    def set_filter_scan(self, limit):
        if limit == 0:
            self.lingering = self.filter_scan
        self.filter_scan = limit

    def scan_limit(self):
        limit, self.lingering = self.filter_scan or self.lingering, 0
        return limit


MUTANTS = (BackLinksNotDirty, ReaddKeepsNeighbourRows, ReaddKeepsUpperSlot, RemoveLeavesMirror, IdCapacityOffByOne,
           UpperPoolOffByOne, RebuildDropsPooledLists, LastChunkNotSynced, MaskClampedToOldIds, ScanSeesReplacedRow, ToggleKeepsRoute)


# ---------------------------------------------------------------------------------------------------------------- the runner
def is_read(op):
    return op[0] in READS


def resolve(trace, op):
    """a mutation -> (method, args) of a Log / an adapter"""
    seed, d, kind = trace["seed"], trace["d"], op[0]
    if kind in ("add", "jump"):
        return "add", (op[1], block_of(seed, op[2], 1, d)[0], -1)
    if kind in ("add_level", "readd_present", "readd_removed", "readd_entry"):
        return "add", (op[1], block_of(seed, op[2], 1, d)[0], op[3])
    if kind in ("remove", "remove_absent", "remove_entry"):
        return "remove", (op[1],)
    if kind == "bulk":
        return "bulk", (bulk_ids(op), block_of(seed, op[1], op[2], d))
    if kind in ("set_build", "set_traversal", "set_filter_scan"):
        return "set", (kind[4:], op[1])
    raise ValueError(kind)


def mask_for(trace, op, model):
    """the eligibility (bool per id, its length = mask_bits) of a masked / filtered / scan read, from the model's state"""
    seed = trace["seed"]
    if op[0] == "scan":
        mkey, over = op[6], op[7]
        present = sorted(model.vec, key=lambda i: -model.order[i])  # newest first
        want = max(1, min((model.filter_scan or 8) + over, len(present)))
        newest = present[:(want + 1) // 2]
        rest = present[len(newest):]
        pick = rng_of(seed, mkey, 3).permutation(len(rest))[:want - len(newest)]
        elig = np.zeros(max(model.n_ids, 1), dtype=bool)
        elig[newest + [rest[int(j)] for j in pick]] = True
        return elig
    mkey, sel, mode = op[6], op[7], op[8]
    bits = max(1, model.n_ids + BITS_MODES[mode])
    return rng_of(seed, mkey, 2).random(bits) < sel


def diff_any(want, got):
    if "error" in want or "error" in got:
        return diff(want, got)
    if "graph" in want:
        (wl, we, wlv, wn), (gl, ge, glv, gn) = want["graph"], got["graph"]
        if wl != gl:
            return f"len {gl}, expected {wl}"
        if tuple(we) != tuple(ge):
            return f"entry point {ge}, expected {we}"
        if wlv != glv:
            bad = [i for i in wlv if glv.get(i) != wlv[i]][:3]
            return f"levels differ at ids {bad}: {[glv.get(i) for i in bad]}, expected {[wlv[i] for i in bad]}"
        for i in wn:
            if wn[i] != gn[i]:
                return f"lists of node {i}: {gn[i]}, expected {wn[i]}"
        return None
    if "vector" in want:
        return None if np.array_equal(want["vector"], got["vector"]) else "vector bits differ"
    return diff(want, got)


def run(trace, adapter, expected=None, counters=True, on_read=None):
    """Apply the trace to the adapter and to a fresh model; compare after every read, and the adapter's mirror_stats() with the
    model's eight predicted counters (counters=False: answers only).  expected: a list with one slot per op that keeps the
    model's answers between runs of one trace.  on_read(step, op, model, adapter).  Returns the model."""
    model = Model(trace)
    ops = trace["ops"]

    def fail(step, op, what):
        head = {k: v for k, v in trace.items() if k != "ops"}
        head["ops"] = list(ops[:step + 1])
        raise Mismatch(f"seed {trace['seed']}, step {step} {op}: {what}\n"
                       f"replay with hnsw_lifecycle.run(TRACE, adapter), TRACE = {head!r}")

    for step, op in enumerate(ops):
        if not is_read(op):
            name, args = resolve(trace, op)
            getattr(model, name)(*args)
            got = capture(lambda: getattr(adapter, name)(*args) and None or {})
            if "error" in got:                                       # (a sync inside a bulk may refuse, as a read's may)
                fail(step, op, f"{name}: {got['error']}, expected no error")
            continue
        kind = op[0]
        cached = expected[step] if expected is not None and expected[step] is not None else {}
        if kind in ("graph", "get_vector"):
            call = (lambda t: t.graph()) if kind == "graph" else (lambda t: t.get_vector(op[1]))
            want = cached.get("one") or capture(lambda: call(model))
            cached["one"] = want
            what = diff_any(want, capture(lambda: call(adapter)))
            if what:
                fail(step, op, what)
        else:
            _, qkey, B, k, ef, near = op[:6]
            q = queries_of(trace, qkey, B, near)
            elig = None if kind == "search" else mask_for(trace, op, model)
            api = kind if kind != "scan" else op[8]
            for route in ("device", "host"):
                if route in cached:                                  # a kept answer: the model still routes the read and syncs its book
                    model.advance_read(api, k, elig, route)
                else:
                    cached[route] = capture(lambda: model.walk(api, q, k, ef, elig, route))
                want = cached[route]
                got = capture(lambda: adapter.walk(api, q, k, ef, elig, route))
                what = diff_any(want, got)
                if what:
                    fail(step, op, f"[{route} route, {model.routes[-1]}] {what}")
        if expected is not None:
            expected[step] = cached
        if counters and hasattr(adapter, "mirror_stats"):
            want, got = model.mirror_stats(), list(adapter.mirror_stats())
            if want != got:
                names = [STAT_NAMES[i] for i in range(8) if want[i] != got[i]]
                fail(step, op, f"mirror_stats {got}, predicted {want} ({', '.join(names)})")
        if on_read is not None:
            on_read(step, op, model, adapter)
    return model


def shrink(trace, make_adapter, log=None, **kw):
    """Drop ops greedily while the failure persists (lifecycle.shrink's loop over this module's run); the failing read stays last.
    Only a Mismatch counts as the failure; any other exception of an attempt is raised, so nothing more is started on an engine
    that reported an error."""
    def fails(ops):
        try:
            run(dict(trace, ops=ops), make_adapter(), **kw)
        except Mismatch as e:
            return int(str(e).split("step ")[1].split(" ")[0]) + 1
        return 0                                                     # (anything else -- an engine error, a failed assertion -- ends the shrinking: it leaves)
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


def coverage(trace):
    """{"pairs": (mutation kind, read kind) with no other mutation between them -- a "scan" read counts only where it took the
    scan route --, "readds": (readd_present | readd_removed, "drawn" | "same" | "lower" | "higher": the op's level against the
    level the id had), "stats": the model's eight counters at the end, "routes": Counter-like dict of the walk reads' routes}"""
    m = Model(trace)
    pairs, readds, last = set(), set(), None
    for op in trace["ops"]:
        if not is_read(op):
            if op[0] in ("readd_present", "readd_removed") and op[1] in m.lvl:
                was = m.lvl[op[1]]
                readds.add((op[0], "drawn" if op[3] < 0 else "same" if op[3] == was else "lower" if op[3] < was else "higher"))
            name, args = resolve(trace, op)
            getattr(m, name)(*args)
            last = op[0]
            continue
        if op[0] in ("graph", "get_vector"):
            r = None
        else:
            elig = None if op[0] == "search" else mask_for(trace, op, m)
            api = op[0] if op[0] != "scan" else op[8]
            r = m.advance_read(api, op[3], elig, "device")
        if last and (op[0] != "scan" or r == "scan"):
            pairs.add((last, op[0]))
    routes = {r: m.routes.count(r) for r in set(m.routes)}
    return {"pairs": pairs, "readds": readds, "stats": m.mirror_stats(), "routes": routes}


# ---------------------------------------------------------------------------------------------------------------- schedules
class _Gen:
    """Deals a schedule while driving a Model of its own, so that every op names real ids, levels and capacities."""
    KS, EFS = (1, 5, 10, 20), (1, 8, 40, 200)

    def __init__(self, seed, metric, d, m, efc=40):
        self.trace = {"seed": int(seed), "metric": int(metric), "d": int(d), "m": int(m), "efc": int(efc), "ops": []}
        self.rng = rng_of(seed, 0, 99)
        self.model = Model(self.trace)
        self.key = 0
        self.near = None
        self.last_id = 0
        self.turn = {}
        self.pairs, self.last = set(), None

    def next_key(self):
        self.key += 1
        return self.key

    def cycle(self, name, choices):
        t = self.turn.get(name, int(self.rng.integers(0, len(choices))))
        self.turn[name] = t + 1
        return choices[t % len(choices)]

    def emit(self, op):
        self.trace["ops"].append(op)
        if is_read(op):
            took = True
            if op[0] not in ("graph", "get_vector"):
                elig = None if op[0] == "search" else mask_for(self.trace, op, self.model)
                api = op[0] if op[0] != "scan" else op[8]
                r = self.model.advance_read(api, op[3], elig, "device")
                took = op[0] != "scan" or r == "scan"
            if self.last and took:
                self.pairs.add((self.last, op[0]))
        else:
            name, args = resolve(self.trace, op)
            getattr(self.model, name)(*args)
            self.last = op[0]
        return op

    # -- mutations
    def fresh(self):
        return self.model.n_ids

    def add(self, i=None, level=None):
        key, i = self.next_key(), self.fresh() if i is None else i
        self.near, self.last_id = (key, 1, 0), i
        return self.emit(("add", i, key) if level is None else ("add_level", i, key, level))

    def readd(self, kind):
        """readd_present / readd_removed at a drawn, the same, a lower and a higher level in turn, each kind on its own turn; the
        id is one whose level can go that way (a removed one is made first where none is left)"""
        m, ep = self.model, self.model.o.entry_point()[0]
        how = self.cycle(kind, ("drawn", "same", "lower", "higher"))
        fits = {"drawn": lambda l: True, "same": lambda l: True, "lower": lambda l: l >= 1, "higher": lambda l: l < MAX_LEVEL}[how]
        pool = [i for i in (m.removed if kind == "readd_removed" else set(m.vec) - {ep}) if fits(m.lvl[i])]
        if not pool:
            i = self.pick(j for j in set(m.vec) - {ep} if fits(m.lvl[j]))
            if kind == "readd_removed":
                self.emit(("remove", i))
        else:
            i = self.pick(pool)
        lvl = m.lvl[i]
        key = self.next_key()
        self.near, self.last_id = (key, 1, 0), i
        return self.emit((kind, i, key, {"drawn": -1, "same": lvl, "lower": lvl - 1, "higher": lvl + 1}[how]))

    def pick(self, ids):
        ids = sorted(ids)
        return ids[int(self.rng.integers(0, len(ids)))]

    def mutate(self, kind):
        m = self.model
        ep = m.o.entry_point()[0]
        if kind == "add":
            return self.add()
        if kind == "add_level":
            return self.add(level=self.cycle("level", (0, 1, 3, MAX_LEVEL, 2, 7)))
        if kind == "jump":
            key, i = self.next_key(), m.n_ids - 1 + max(m.book.cap_ids, 1) + int(self.rng.integers(1, 40))
            self.near, self.last_id = (key, 1, 0), i
            return self.emit(("jump", i, key))
        if kind in ("readd_present", "readd_removed"):
            return self.readd(kind)
        if kind == "readd_entry":
            key = self.next_key()
            self.near, self.last_id = (key, 1, 0), ep
            return self.emit((kind, ep, key, 0))
        if kind in ("remove", "remove_entry"):
            i = ep if kind == "remove_entry" else self.pick(set(m.vec) - {ep})
            self.near, self.last_id = None, i
            return self.emit((kind, i))
        if kind == "remove_absent":
            i = self.pick(m.removed) if m.removed and self.rng.random() < 0.5 else m.n_ids + 5
            self.near, self.last_id = None, i
            return self.emit((kind, i))
        if kind == "bulk":
            return self.bulk(self.cycle("bulk", BULK_SIZES), share=self.cycle("share", (0.0, 0.1, 0.0, 0.05)), twice=self.cycle("twice", (False, True, False)))
        if kind == "set_build":
            return self.emit((kind, not m.frontier))
        if kind == "set_traversal":
            return self.emit((kind, not m.host_only))
        if kind == "set_filter_scan":
            if m.filter_scan:
                return self.scan_off()
            return self.emit((kind, self.cycle("limit", (8, 5))))
        raise ValueError(kind)

    def scan_off(self):
        """the toggle that ends the scan, and at once a mask the scan would have taken, with k = ef = 1: the walk is not exhaustive"""
        op = self.emit(("set_filter_scan", 0))
        self.emit(("scan", self.next_key(), 3, 1, 1, None, self.next_key(), 0, "masked"))
        return op

    def bulk(self, n, share=0.0, twice=False):
        m, key, first = self.model, self.next_key(), self.fresh()
        repl = {}
        seen = sorted(set(m.vec) | m.removed)
        for p in range(n):
            if seen and self.rng.random() < share:
                repl[p] = self.pick(seen)
        if twice and n >= 3:
            p = int(self.rng.integers(1, n))
            repl[p] = first + int(self.rng.integers(0, p))
            repl.pop(repl[p] - first, None)                          # (the first occurrence stays the fresh id itself)
        last = n - 1
        again = [i for i in repl.values() if i in seen]
        self.near, self.last_id = (key, n, last), again[0] if again else first + last      # get_vector: a replaced id first
        return self.emit(("bulk", key, n, first, tuple(sorted(repl.items()))))

    # -- reads
    def q(self):
        near = self.near if self.near is not None and self.rng.random() < 0.7 else None
        k = self.cycle("k", self.KS)
        return self.next_key(), self.cycle("B", (1, 2, 1, 3)), k, self.cycle("ef", self.EFS), near

    def read(self, kind):
        if kind == "search":
            return self.emit(("search",) + self.q())
        if kind in ("masked", "filtered"):
            return self.emit((kind,) + self.q() + (self.next_key(), self.cycle("sel" + kind, SELECTIVITIES), self.cycle("bits" + kind, (0, 1, 2))))
        if kind == "scan":                                           # at the limit; every other time also one node above it: the walk answers
            op = self.emit(("scan",) + self.q() + (self.next_key(), 0, self.cycle("api", ("masked", "filtered"))))
            if self.cycle("over", (False, True)):
                self.emit(("scan",) + self.q() + (self.next_key(), 1, self.cycle("api", ("masked", "filtered"))))
            return op
        if kind == "graph":
            return self.emit(("graph",))
        if kind == "get_vector":
            return self.emit(("get_vector", self.last_id))
        raise ValueError(kind)

    def base(self, n):
        self.bulk(n)
        self.emit(("search", self.next_key(), 2, 10, 40, None))
        self.emit(("set_filter_scan", 8))                            # on from the start: "scan" reads take the scan route
        self.emit(("graph",))

    def mix(self, limit=150):
        """mutations and reads until every (mutation, read) pair has occurred"""
        todo = [(a, b) for a in MUTATIONS for b in READS]
        while True:
            missing = [p for p in todo if p not in self.pairs]
            if not missing or len(self.trace["ops"]) >= limit:
                break
            kinds = sorted({a for a, _ in missing}, key=MUTATIONS.index)
            kind = kinds[int(self.rng.integers(0, len(kinds)))]
            wanted = [b for a, b in missing if a == kind]
            if "scan" in wanted and kind != "set_filter_scan" and not self.model.filter_scan:
                self.emit(("set_filter_scan", 8))
            if kind == "set_filter_scan" and "scan" in wanted and self.model.filter_scan:
                self.scan_off()                                      # the pair needs the toggle that switches the scan ON
            self.mutate(kind)
            order = self.rng.permutation(len(wanted))
            for j in order[:3]:
                self.read(wanted[int(j)])
        return self

    def cosine_zero(self):
        """one all-zero query through every route (InvalidVector under Cosine)"""
        for kind, extra in (("search", ()), ("masked", (self.next_key(), 1.0, 1)), ("masked", (self.next_key(), 0.0, 1)),
                            ("filtered", (self.next_key(), 0.5, 1)), ("scan", (self.next_key(), 0, "masked")),
                            ("scan", (self.next_key(), 0, "filtered"))):
            self.emit((kind, ZERO_QUERY, 2, 5, 8, None) + extra)


def schedule(seed, metric, d, m, base, efc=40):
    g = _Gen(seed, metric, d, m, efc)
    g.base(base)
    g.mix()
    if metric == COSINE:
        if not g.model.filter_scan:
            g.emit(("set_filter_scan", 8))
        g.cosine_zero()
    return g.trace


def near_cap(g):
    b = g.model.book
    return b.cap_ids, b.cap_upper - b.used


def walk_after(g, turn):
    """a walk that looks for the node just added: plain, masked and filtered in turn, ef small enough to depend on the descent"""
    k, ef = ((1, 1), (5, 8), (3, 40))[turn % 3]
    if turn % 3 == 0:
        g.emit(("search", g.next_key(), 1, k, ef, g.near))
    else:
        g.emit((("masked", "filtered")[turn % 2], g.next_key(), 1, k, ef, g.near, g.next_key(), 1.0, turn % 3))


def edge_ids(seed=101, metric=EUCLID):
    """single fresh adds, a search after every one, up to and past cap_ids: the ids cap_ids - 1, cap_ids, cap_ids + 1"""
    g = _Gen(seed, metric, 8, 4)
    g.base(300)
    for t in range(12):
        g.add()
        walk_after(g, t)
    cap = g.model.book.cap_ids
    for t, i in enumerate((cap - 3, cap - 2, cap - 1, cap, cap + 1, cap + 2)):
        g.add(i)
        walk_after(g, 0 if i == cap else t)
    cap2 = g.model.book.cap_ids                                      # of the rebuild the id `cap` forced
    for t, i in enumerate((cap2 - 1, cap2, cap2 + 1)):
        g.add(i)
        walk_after(g, t)
    g.emit(("graph",))
    return g.trace


def edge_pool(seed=102, metric=COSINE):
    """add_level at 15 until the pool is within one node of cap_upper, then exactly to it, then one slot past it"""
    g = _Gen(seed, metric, 8, 4)
    g.base(300)
    t = 0
    while near_cap(g)[1] >= 2 * MAX_LEVEL:
        g.add(level=MAX_LEVEL)
        walk_after(g, t)
        t += 1
    left = near_cap(g)[1]                                            # 15 .. 29
    if left > MAX_LEVEL:
        g.add(level=left - MAX_LEVEL)                                # within one node: exactly 15 slots are left
        walk_after(g, 1)
    g.add(level=MAX_LEVEL)                                           # exactly to it: the pool is full, still a scatter
    walk_after(g, 0)
    assert near_cap(g)[1] == 0 and g.model.book.c[3] == 0
    g.add(level=1)                                                   # one slot past it: the rebuild for the pool
    walk_after(g, 0)
    for t in range(3):
        g.add(level=MAX_LEVEL)
        walk_after(g, t)
    g.emit(("graph",))
    return g.trace


def edge_jump(seed=103, metric=DOT):
    """a jump, adds below and above the old capacity, then a re-add whose higher level no longer fits the pool"""
    g = _Gen(seed, metric, 8, 4)
    g.base(300)
    old = g.model.book.cap_ids
    g.mutate("jump")
    walk_after(g, 0)
    for t, i in enumerate((300, old - 1, old, old + 1, g.model.n_ids)):
        g.add(i)
        walk_after(g, t)
    m = g.model

    def readd_pooled(nth):
        """a node with a slot in the middle of the pool comes back 15 levels high; then descents (k = ef = 1) towards the nodes
        whose slots lie behind its old one, and towards their layer-1 neighbours"""
        pooled = [i for i in sorted(m.vec) if 1 <= m.lvl[i] < 3 and i < 300 and m.ver[i] == 1]
        x = pooled[len(pooled) * nth // 4]
        after = [i for i in sorted(m.vec) if m.lvl[i] >= 1 and i > x][:MAX_LEVEL]
        around = tuple(dict.fromkeys(j for y in after for j in [y] + (m.o.neighbors(y, 1) or []) if j < 300 and j != x and m.ver[j] == 1))[:48]
        key = g.next_key()
        g.near, g.last_id = (key, 1, 0), x
        g.emit(("readd_present", x, key, MAX_LEVEL))
        g.emit(("search", g.next_key(), len(around), 1, 1, (1, 300, around)))
        walk_after(g, 1)
        g.emit(("get_vector", x))
    readd_pooled(2)                                                  # the new top of the graph: its upper lists are empty
    t = 0
    while near_cap(g)[1] >= MAX_LEVEL:
        g.add(level=MAX_LEVEL)
        walk_after(g, t)
        t += 1
    readd_pooled(1)                                                  # its 15 lists no longer fit what is left of the pool
    g.add(level=MAX_LEVEL)
    walk_after(g, 1)
    while near_cap(g)[1] >= MAX_LEVEL:
        g.add(level=MAX_LEVEL)
        walk_after(g, 2)
    g.add(level=MAX_LEVEL)                                           # no longer fits: the rebuild for the pool
    walk_after(g, 0)
    g.emit(("graph",))
    return g.trace


PINNED = {
    "euclid d8 m4 n300": lambda: schedule(11, EUCLID, 8, 4, 300),
    "cosine d16 m6 n600": lambda: schedule(12, COSINE, 16, 6, 600),
    "dot d33 m16 n1500": lambda: schedule(13, DOT, 33, 16, 1500),
    "euclid d33 m6 n900": lambda: schedule(14, EUCLID, 33, 6, 900),
    "cosine d8 m4 n400": lambda: schedule(15, COSINE, 8, 4, 400),
    "dot d16 m4 n500": lambda: schedule(16, DOT, 16, 4, 500),
    "euclid d16 m16 n1000": lambda: schedule(17, EUCLID, 16, 16, 1000),
    "cosine d33 m16 n700": lambda: schedule(18, COSINE, 33, 16, 700),
    "dot d8 m6 n300": lambda: schedule(19, DOT, 8, 6, 300),
    "edge ids": edge_ids,
    "edge pool": edge_pool,
    "edge jump": edge_jump,
}
EDGES = ("edge ids", "edge pool", "edge jump")
_TRACES, _SLOTS = {}, {}


def pinned(name):
    if name not in _TRACES:
        _TRACES[name] = PINNED[name]()
    return _TRACES[name]


def slots(name):
    """the `expected` list of run() for a pinned trace: computed by the first run, shared by every later one"""
    return _SLOTS.setdefault(name, [None] * len(pinned(name)["ops"]))


def edge_conditions(name, stats, trace):
    """what an edge schedule must reach, on any list of the eight counters (the model's, or the device's own)"""
    if name in ("edge ids", "edge jump"):
        assert stats[2] >= 1, (name, stats)
    if name in ("edge pool", "edge jump"):
        assert stats[3] >= 1, (name, stats)
    assert stats[1] + stats[2] + stats[3] == stats[0], stats
    singles = sum(1 for op in trace["ops"] if op[0] in ("add", "add_level", "jump"))
    assert stats[4] >= singles - (stats[0] - 1), (name, stats, singles)   # every fresh single add is scattered, or starts a rebuild


# ---------------------------------------------------------------------------------------------------------------- the adapter over the engine
class GpuHnswAdapter:
    """GpuHnswIndex plus a MetaTable whose column 0 holds a read's eligibility as codes 0 / 1.  A device-route walk asserts that
    the device-resident search answered it (device_queries grew, host_redone stayed 0)."""

    def __init__(self, vdb, trace):
        self.vdb = vdb
        self.ix = vdb.GpuHnswIndex(vdb.DistanceMetric(trace["metric"]), vdb.HnswParams.new(trace["m"], trace["efc"], 50), seed=trace["seed"])
        self.table = vdb.MetaTable(0)
        self.host_only, self.n_ids, self.device_walked = False, 0, 0

    def close(self):
        self.table.close()

    def add(self, i, v, level=-1):
        self.ix.add(int(i), self.vdb.Vector(v), level=int(level))
        self.n_ids = max(self.n_ids, int(i) + 1)

    def bulk(self, ids, rows):
        self.ix.build_batch((np.array(ids, dtype=U64), rows))
        self.n_ids = max(self.n_ids, max(ids) + 1)

    def remove(self, i):
        self.ix.remove(int(i))

    def set(self, name, value):
        if name == "build":
            self.ix.set_build(bool(value))
        elif name == "traversal":
            self.host_only = bool(value)
            self.ix.set_traversal(self.host_only)
        else:
            self.ix.set_filter_scan(int(value))

    def _search(self, api, q, k, ef, elig):
        if elig is None:
            return self.ix.search_batch_arrays(q, k, ef)
        if api == "masked":
            out = np.zeros((elig.size + 63) // 64 * 8, dtype=np.uint8)
            pb = np.packbits(elig, bitorder="little")
            out[:pb.size] = pb
            return self.ix.search_batch_arrays(q, k, ef, id_mask=out.view(U64), mask_bits=elig.size)
        self.table.set_codes(0, 0, elig.astype(np.int32))
        self.table.set_present(0, elig.size, True)
        with self.table.compile([(self.vdb.MetaTable.EQ, 0, 1)], elig.size) as cm:
            return self.ix.search_batch_arrays(q, k, ef, compiled_mask=cm)

    def walk(self, api, q, k, ef, elig, route):
        before = self.ix.stats()
        if route == "device":
            self.device_walked = 0                                   # (a refused query walks nothing)
        self.ix.set_traversal(route == "host")
        try:
            gi, gd, gc = self._search(api, q, k, ef, elig)
        except self.vdb.InvalidVector:
            raise Predicted("InvalidVector")
        finally:
            self.ix.set_traversal(self.host_only)
        after = self.ix.stats()
        assert after["host_redone"] == 0, after
        walked = after["device_queries"] - before["device_queries"]
        if route == "host":
            assert walked == 0, (before, after)
        else:
            self.device_walked = walked
        return answer_of([(gi[b, :int(c)], gd[b, :int(c)]) for b, c in enumerate(gc)])

    def graph(self):
        ix = self.ix
        ids = [i for i in range(self.n_ids) if ix.level(i) >= 0]
        levels = {i: ix.level(i) for i in ids}
        return {"graph": (ix.len(), ix.entry_point(), levels, {i: [ix.neighbors(i, l) for l in range(levels[i] + 1)] for i in ids})}

    def get_vector(self, i):
        v = self.ix.get_vector(int(i))
        if v is None:
            raise Predicted("VectorNotFound")
        return {"vector": np.ascontiguousarray(v.data, dtype=F32).view(np.uint32).copy()}

    def mirror_stats(self):
        s = self.ix.mirror_stats()
        return [s[n] for n in STAT_NAMES]


def run_gpu(vdb, trace, expected=None):
    """run() over a GpuHnswAdapter.  A read the model routes to the walk must have been answered by the device-resident search on
    its device pass, query for query; a scan, an empty mask and a refused query by none.  -> (model, the device's final
    mirror_stats, queries walked on the device)"""
    ad = GpuHnswAdapter(vdb, trace)
    walked = [0]

    def on_read(step, op, model, adapter):
        if op[0] in ("graph", "get_vector"):
            return
        r = model.routes[-1]
        refused = model.zero_refused(queries_of(trace, op[1], op[2], op[5]))
        want = op[2] if r == "walk" and not refused else 0
        assert ad.device_walked == want, f"step {step} {op}: {ad.device_walked} queries walked on the device, expected {want} ({r})"
        walked[0] += want
    try:
        model = run(trace, ad, expected=expected, on_read=on_read)
        return model, ad.mirror_stats(), walked[0]
    finally:
        ad.close()


def shrink_gpu(vdb, trace, log=None):
    """shrink() over fresh GpuHnswAdapters: the smallest trace found that still fails on the device, or None"""
    class Fresh(GpuHnswAdapter):
        def __del__(self):
            self.close()
    return shrink(trace, lambda: Fresh(vdb, trace), log=log)

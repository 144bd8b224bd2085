"""Every mutation of the rows under the SPLIT layout rule: one scripted schedule, the rule as a state machine, and
a CPU stand-in of the store that keeps its rows as the BYTES of either layout.  No GPU, no import of the product.

  Rule          what layout() must read after every step: staged appends, tombstones, compactions, re-allocations, searches,
                reads by id, a refusal and when it is forgotten.
  run_schedule  add, upsert, remove, compact, shrink-compact and refill to the same row count, growth across a re-allocation, a
                fall below the screening floor and back, a late non-finite row that is removed again -- a plain search (and a read
                by id) after each; the subject must equal its mode-0 twin and the oracle over the row log bit for bit, and its
                layout() the Rule, after EVERY step.  tests/test_gpu_split_paths.py runs it over two GpuFlatIndex handles at the
                engine's floor of 65 536 rows, tests/test_split_schedule_cpu.py over two SimIndex at a floor of 1024.
  SimIndex      the store in numpy: csrc/row_split.h restated (split_hi / split_lo / split_join on 16-bit words), rows_f32 /
                rows_mut / rows_to_split as vdb_store.cpp has them, searches answered by the oracle over the rows JOINED from the
                bytes as they lie.  Its MUTANTS are the three ways this layout goes wrong without an error anywhere: a reader that
                takes the bytes as floats, an append written into split rows, a refusal forgotten."""
import numpy as np

import by_id_data as bd
import oracle

F32, SPLIT = 0, 1
RUN = 2                                            # the adaptive rule's run in these schedules (debug_set_split_after)
U64 = np.uint64


def round_up(x, m):
    return (x + m - 1) // m * m


def grown(cap, need):
    """vdb_store.cpp grow(): at least the need, at least twice the old capacity, at least 1024 rows, whole 256-row blocks"""
    return cap if need <= cap else round_up(max(need, 2 * cap, 1024), 256)


class Rule:
    """The layout rule of DESIGN 4.3 as a state machine over what a schedule does to ONE plain index.  It holds for one sample
    size -- depths of at most 58 and fewer than 262 144 rows -- so the compact sample copy is keyed by the row count alone.
    forward / back / refusals count what it predicted."""

    def __init__(self, mode, n, floor=65536):
        self.mode, self.floor, self.layout, self.conv, self.streak, self.refused = mode, floor, F32, 0, 0, False
        self.n, self.staged, self.dead, self.sample_n = n, 0, 0, None
        self.cap = grown(0, n)
        self.bad_staged = self.bad_stored = False                   # a non-finite element among the staged / the uploaded rows
        self.forward = self.back = self.refusals = 0

    def expect(self):
        return self.layout, self.conv

    def reader(self):                                               # rows_f32()
        self.streak = 0
        if self.layout == SPLIT:
            self.layout, self.conv, self.back = F32, self.conv + 1, self.back + 1

    def mutate(self):                                               # rows_mut()
        self.refused = False
        self.reader()

    def add(self, rows=1, overwrites=0, bad=False):                 # staged on the host; an id already stored is tombstoned first
        self.staged += rows
        self.bad_staged |= bad
        if overwrites:
            self.remove(overwrites)

    def remove(self, rows=1):                                       # kill_row: the live bitmask and the count, not the rows
        self.dead += rows
        self.streak = 0

    def flush(self):                                                # what every read and every compaction does first
        if self.staged:
            self.mutate()                                           # (a re-allocation reads the old rows as f32 rows too: one conversion)
            self.n, self.staged = self.n + self.staged, 0
            self.cap = grown(self.cap, self.n)
            self.bad_stored, self.bad_staged = self.bad_stored or self.bad_staged, False

    def compact(self, shrink=False, bad_left=False):
        self.flush()
        if self.dead:
            self.mutate()
            self.n, self.dead, self.sample_n, self.bad_stored = self.n - self.dead, 0, None, bad_left
        cap = round_up(max(self.n, 1024), 256)
        if shrink and cap < self.cap:
            self.cap = cap
            self.reader()                                           # the smaller store is filled from f32 rows

    def search(self, nq=9, handed_over=False, by_id=False):
        self.flush()
        if by_id:
            self.reader()                                           # the gather of the stored rows
        if self.n < self.floor:
            return self.reader()                                    # below the screening floor every tier reads f32 rows
        if self.sample_n != self.n or self.mode == 0:
            self.reader()                                           # the compact sample copy is rebuilt from f32 rows (mode 0: no split rows)
            self.sample_n = self.n
        if nq <= 256 and self.mode != 0:
            if self.layout == F32 and not self.refused and (self.mode == 2 or self.streak >= RUN):
                self.conv, self.forward = self.conv + 1, self.forward + 1
                if self.bad_stored:                                 # found out: straight back, and not again until the rows change
                    self.refused, self.conv, self.back, self.refusals = True, self.conv + 1, self.back + 1, self.refusals + 1
                else:
                    self.layout = SPLIT
            self.streak += 1
        if handed_over:
            self.reader()


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
                                    for x, y in zip(a, b))


def check_oracle(metric, rows, q, k, res, qsel, live=None, ids=None):
    gi, gd, gc = res
    for b in qsel:
        oi, od = oracle.flat_search(metric, rows, q[b], k, ids=ids, live=live)
        assert gc[b] == len(oi), (b, gc[b], len(oi))
        assert np.array_equal(gi[b, :len(oi)], oi), (b, gi[b, :len(oi)], oi)
        assert np.array_equal(gd[b, :len(oi)].view(np.uint32), od.view(np.uint32)), (b, gd[b, :len(oi)], od)


def run_schedule(a, b, metric, mode, base, queries, floor=65536):
    """a: the mode-0 twin, b: the subject under `mode` (2 or "adaptive"), both already holding the rows `base` under the ids
    0 .. n - 1.  Either is anything with add(id, v) / add_bulk(rows, ids) / remove(id) / compact(shrink) / search(q, k) /
    by_id(ids, k) -- the last two returning ("ok", ids, dists, counts) or ("error", class name, message) -- and layout(),
    last_stats(), capacity().  Returns the Rule at the end."""
    k = 10
    n0, d = base.shape
    assert n0 == floor + 37
    q = np.ascontiguousarray(queries[:9])
    rng = np.random.default_rng([77, metric])
    rule = Rule(mode, n0, floor)
    log_rows, log_ids, alive = [base], [np.arange(n0, dtype=U64)], [np.ones(n0, dtype=np.uint8)]
    next_id = [10 ** 6]

    def rows_ids_live():
        return np.concatenate(log_rows), np.concatenate(log_ids), np.concatenate(alive)

    def agree(step):
        assert a.layout() == (F32, 0), step
        assert b.layout() == rule.expect(), (step, metric, mode, "predicted", rule.expect(), "seen", b.layout())

    def kill(ids, count=True):
        ids, killed = np.asarray(ids, dtype=U64), 0
        for part_ids, part_alive in zip(log_ids, alive):
            hit = np.isin(part_ids, ids) & (part_alive != 0)
            part_alive[hit] = 0
            killed += int(hit.sum())
        if count and killed:
            rule.remove(killed)
        return killed

    def append(rows, ids, bad=False):
        again = kill(ids, count=False)
        log_rows.append(np.ascontiguousarray(rows, dtype=np.float32))
        log_ids.append(np.asarray(ids, dtype=U64))
        alive.append(np.ones(len(ids), dtype=np.uint8))
        rule.add(len(ids), overwrites=again, bad=bad)

    def add_one(v, id, step, bad=False):
        append(v[None, :], [id], bad=bad)
        for ix in (a, b):
            ix.add(int(id), v)
        agree(step)

    def add_many(m, step):
        rows = rng.standard_normal((m, d)).astype(np.float32)
        ids = np.arange(next_id[0], next_id[0] + m, dtype=U64)
        next_id[0] += m
        append(rows, ids)
        for ix in (a, b):
            ix.add_bulk(rows, ids)
        agree(step)

    def remove(ids, step):
        ids = sorted(set(int(i) for i in ids))
        kill(ids)
        for ix in (a, b):
            for i in ids:
                ix.remove(i)
        agree(step)

    def remove_many(m, step):
        rows, ids, live = rows_ids_live()
        remove(rng.choice(ids[live != 0], m, replace=False), step)

    def compact(step, shrink=False, bad_left=False):
        for ix in (a, b):
            ix.compact(shrink)
        rule.compact(shrink, bad_left)
        agree(step)

    def check(step, times=1, screened=1):
        for t in range(times):
            ra, rb = a.search(q, k), b.search(q, k)
            st = b.last_stats()
            rule.search(len(q), handed_over=bool(st["f32_tier_queries"] or st["exact_queries"]))     # (also when the search then fails)
            assert ra[0] == rb[0] and (same(ra[1:], rb[1:]) if ra[0] == "ok" else ra[1:] == rb[1:]), (step, t, ra[:2], rb[:2])
            if rb[0] == "ok":
                assert st["bf16_screen"] == screened, (step, st)
            agree((step, t, st))
        if rb[0] == "ok":
            rows, ids, live = rows_ids_live()
            check_oracle(metric, rows, q, k, rb[1:], [0, 8], live=live, ids=ids)
        return rb

    def by_id(step):
        rows, ids, live = rows_ids_live()
        at = np.nonzero(live)[0][[3, 1000, -1]]
        ra, rb = a.by_id(ids[at], k), b.by_id(ids[at], k)
        rule.search(len(at), by_id=True)
        assert ra[0] == rb[0] == "ok" and same(ra[1:], rb[1:]), (step, ra[:2], rb[:2])
        bd.check(rb[1:], bd.expected(metric, rows, [int(r) for r in at], k, ids=ids, live=live), step)
        agree(step)

    check("fresh", times=RUN + 1)
    assert b.layout()[0] == SPLIT
    # ---- add, upsert, remove
    add_one(q[0] + np.float32(0.01) * rng.standard_normal(d).astype(np.float32), next_id[0], "add")
    next_id[0] += 1
    rb = check("after add")
    assert rb[1][0, 0] == next_id[0] - 1 or metric == 2              # (the new row is query 0's nearest; under Dot the longest row is)
    add_one(q[1] + np.float32(0.01) * rng.standard_normal(d).astype(np.float32), 5, "upsert")
    rb = check("after upsert")
    assert rb[1][1, 0] == 5 or metric == 2
    remove([int(x) for x in rb[1][0, :3]] + list(range(100, 120)), "remove")       # query 0 loses its three nearest
    check("after remove", times=RUN + 1)
    assert b.layout()[0] == SPLIT
    by_id("by id over split rows")
    # ---- compact (still above the floor), then a shrinking compaction and a refill to the same row count
    check("before compact", times=RUN + 1)
    compact("compact")
    assert rule.n >= floor
    check("after compact", times=RUN + 1)
    n_before = rule.n
    remove_many(floor // 72, "remove many")
    compact("shrink-compact", shrink=True)
    add_many(n_before - rule.n, "refill")
    check("after refill", times=RUN + 1)
    assert rule.n == n_before and b.layout()[0] == SPLIT
    # ---- growth across a re-allocation
    cap = b.capacity()
    assert cap == rule.cap
    add_many(cap - rule.n + 300, "grow")
    check("after growth", times=RUN + 1)
    assert b.capacity() == rule.cap > cap and b.layout()[0] == SPLIT
    # ---- below the screening floor and back
    rows, ids, live = rows_ids_live()
    remove_many(int(live.sum()) - (floor - floor // 12), "fall")
    compact("compact below the floor")
    check("below the floor", times=2, screened=0)
    assert b.layout()[0] == F32
    add_many(n0 - rule.n, "back above the floor")
    check("above the floor again", times=RUN + 1)
    assert b.layout()[0] == SPLIT
    # ---- a non-finite row arrives late: a refusal that holds until the rows change.  While the row is alive the engine hands
    # every query on to the tiers that read f32 rows (nothing certifies beside an infinite norm), which resets the adaptive count
    # after every search: mode 2 is refused by the first search, the adaptive rule never gets to try.  Once the row is a tombstone
    # the searches certify again and the adaptive rule tries too -- the conversion walks the rows, not the live bits: refused.
    bad = base[17].copy()
    bad[3] = np.inf
    add_one(bad, next_id[0], "late inf", bad=True)
    check("with the inf row", times=2)
    assert b.layout()[0] == F32 and (rule.refusals == 1 or mode != 2)
    remove([next_id[0]], "remove the inf row")
    check("tombstoned, still stored", times=RUN + 2)
    assert rule.refused and rule.refusals == 1 and b.layout()[0] == F32
    compact("compact the inf row away")
    check("retry", times=RUN + 1)
    assert b.layout()[0] == SPLIT and not rule.refused
    assert rule.forward >= 6 and rule.back >= 6 and rule.refusals == 1, (rule.forward, rule.back, rule.refusals)
    return rule


# ================================================================== the store in numpy
def split_hi(bits):
    """csrc/row_split.h: the upper half plus bit 15, modulo 2^16"""
    bits = np.asarray(bits, dtype=np.uint32)
    return (((bits >> 16) + ((bits >> 15) & 1)) & 0xffff).astype(np.uint16)


def split_lo(bits):
    return (np.asarray(bits, dtype=np.uint32) & 0xffff).astype(np.uint16)


def split_join(hi, lo):
    hi, lo = np.asarray(hi, dtype=np.uint32), np.asarray(lo, dtype=np.uint32)
    return ((((hi - (lo >> 15)) & 0xffff) << 16) | lo).astype(np.uint32)


def split_nonfinite(bits):
    return (np.asarray(bits, dtype=np.uint32) & 0x7f800000) == 0x7f800000


MUTANTS = ("reader_takes_bytes", "append_into_split", "refusal_forgotten")


class SimIndex:
    """One plain index as vdb_store.cpp / vdb_search.cpp keep it, in numpy.  `mem` is the row store as 16-bit words, [rows][2 ld]:
    F32 -- the ld floats of a row; SPLIT -- ld hi words, then ld lo words.  Every reader goes through rows_f32() / rows_mut(),
    except a search over SPLIT rows, which joins the two planes (the re-rank kernels' fold).  mutant: one of MUTANTS."""

    def __init__(self, metric, mode, rows, floor, mutant=None):
        assert mutant in (None,) + MUTANTS
        self.metric, self.mode, self.floor, self.mutant = metric, mode, floor, mutant
        self.d = rows.shape[1]
        self.ld = round_up(self.d, 32)
        self.mem = np.zeros((0, 2 * self.ld), dtype=np.uint16)
        self.ids, self.live = np.zeros(0, dtype=U64), np.zeros(0, dtype=np.uint8)
        self.pending, self.pending_ids = [], []
        self.layout_, self.conv, self.streak, self.refused, self.sample_n, self.cap = F32, 0, 0, False, None, 0
        self.stats = dict(bf16_screen=0, f32_tier_queries=0, exact_queries=0)
        self.add_bulk(rows, np.arange(len(rows), dtype=U64))

    # -- the layout (vdb_store.cpp)
    def _convert(self, forward):
        ld = self.ld
        if forward:
            bits = np.ascontiguousarray(self.mem).view(np.uint32)
            self.mem = np.concatenate([split_hi(bits), split_lo(bits)], axis=1)
        else:
            self.mem = np.ascontiguousarray(split_join(self.mem[:, :ld], self.mem[:, ld:])).view(np.uint16)
        self.layout_ = SPLIT if forward else F32
        self.conv += 1

    def _as_floats(self):
        """the store's bytes taken as ld floats a row: right for F32 rows only"""
        return np.ascontiguousarray(self.mem).view(np.uint32).view(np.float32)[:, :self.d]

    def rows_f32(self):
        self.streak = 0
        if self.layout_ == SPLIT:
            self._convert(False)
        return self._as_floats()

    def rows_mut(self):
        self.refused = False
        return self.rows_f32()

    def rows_to_split(self):
        if self.layout_ == SPLIT or self.refused or not len(self.mem) or self.ld % 64:
            return
        bad = bool(split_nonfinite(np.ascontiguousarray(self.mem).view(np.uint32)).any())
        self._convert(True)
        if bad:
            self.refused = True
            self._convert(False)

    # -- mutations
    def add(self, id, v):
        self.remove(id)
        self.pending.append(np.asarray(v, dtype=np.float32))
        self.pending_ids.append(int(id))

    def add_bulk(self, rows, ids):
        for i, v in zip(np.asarray(ids, dtype=U64).tolist(), np.asarray(rows, dtype=np.float32)):
            self.add(i, v)

    def remove(self, id):
        hit = (self.ids == U64(id)) & (self.live != 0)
        if hit.any():
            self.live[hit] = 0
            self.streak = 0
        for j, pid in enumerate(self.pending_ids):                   # (a staged row of that id dies too)
            if pid == int(id) and self.pending[j] is not None:
                self.pending[j] = None

    def _flush(self):
        if not self.pending:
            return
        new = np.zeros((len(self.pending), self.ld), dtype=np.float32)
        alive = np.ones(len(self.pending), dtype=np.uint8)
        for j, v in enumerate(self.pending):
            if v is None:
                alive[j] = 0
            else:
                new[j, :self.d] = v
        words = new.view(np.uint32).view(np.uint16).reshape(len(new), 2 * self.ld)
        self.cap = grown(self.cap, len(self.mem) + len(new))
        if self.mutant == "append_into_split" and self.layout_ == SPLIT:
            self.mem = np.concatenate([self.mem, words])              # f32 bytes behind split rows ...
            self.rows_mut()                                          # ... and the whole store "converted back"
        else:
            self.rows_mut()
            self.mem = np.concatenate([self.mem, words])
        self.ids = np.concatenate([self.ids, np.array(self.pending_ids, dtype=U64)])
        self.live = np.concatenate([self.live, alive])
        self.pending, self.pending_ids = [], []

    def compact(self, shrink=False):
        self._flush()
        if not self.live.all():
            self.rows_mut()
            keep = self.live != 0
            self.mem, self.ids, self.live = self.mem[keep], self.ids[keep], self.live[keep]
            self.sample_n = None
        cap = round_up(max(len(self.mem), 1024), 256)
        if shrink and cap < self.cap:
            self.cap = cap
            self.rows_f32()

    # -- reads
    def _joined(self):
        """the f32 rows whatever the layout: what the filter pass's candidates are re-ranked with"""
        if self.layout_ == F32:
            return self._as_floats()
        return split_join(self.mem[:, :self.ld], self.mem[:, self.ld:]).view(np.float32)[:, :self.d]

    def _tiers(self, q, k):
        n = len(self.mem)
        self.stats = dict(bf16_screen=int(n >= self.floor), f32_tier_queries=0, exact_queries=0)
        if n < self.floor:
            rows = self.rows_f32()
        else:
            if self.sample_n != n:
                self.rows_f32()
                self.sample_n = n
            if len(q) <= 256:
                if self.layout_ == F32 and not self.refused and (self.mode == 2 or (self.mode == "adaptive" and self.streak >= RUN)):
                    self.rows_to_split()
                self.streak += 1
            rows = self._joined()
        try:
            res = oracle.search_batch(self.metric, np.ascontiguousarray(rows), q, k, ids=self.ids, live=self.live)
        except oracle.OracleError as e:
            return ("error", "OracleError", str(e.code))
        finally:
            if self.mutant == "refusal_forgotten":
                self.refused = False
        gi = np.zeros((len(q), k), dtype=U64)
        gd = np.zeros((len(q), k), dtype=np.float32)
        gc = np.zeros(len(q), dtype=np.uintp)
        for b, (oi, od) in enumerate(res):
            gi[b, :len(oi)], gd[b, :len(oi)], gc[b] = oi, od, len(oi)
        return ("ok", gi, gd, gc)

    def search(self, q, k):
        self._flush()
        return self._tiers(np.ascontiguousarray(q, dtype=np.float32), k)

    def by_id(self, ids, k):
        self._flush()
        at = [int(np.nonzero((self.ids == U64(i)) & (self.live != 0))[0][-1]) for i in ids]
        rows = self._as_floats() if self.mutant == "reader_takes_bytes" else self.rows_f32()     # the gather of the stored rows
        q = np.ascontiguousarray(rows[at])
        out = self._tiers(q, k + 1)
        if out[0] != "ok":
            return out
        gi, gd, gc = (np.zeros((len(at), k), dtype=U64), np.zeros((len(at), k), dtype=np.float32), np.zeros(len(at), dtype=np.uintp))
        for b, own in enumerate(ids):
            oi, od, _, _ = bd.strike(out[1][b, :int(out[3][b])], out[2][b, :int(out[3][b])], own, k)
            gi[b, :len(oi)], gd[b, :len(oi)], gc[b] = oi, od, len(oi)
        return ("ok", gi, gd, gc)

    def layout(self):
        return self.layout_, self.conv

    def last_stats(self):
        return self.stats

    def capacity(self):
        return self.cap

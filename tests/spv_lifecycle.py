"""Stateful lifecycle tests of the sparse-vector index: a model, a schedule generator and a runner (no GPU, no import of the product),
after tests/lifecycle.py.

A TRACE is plain data: {"seed", "ops": [tuple, ...]}.  Every vector, id permutation, mask and query is derived from (trace seed, the
key an op carries), so a trace can be printed and replayed with run(trace, adapter).  run() applies every op to the adapter and to
the MODEL and compares after every read: ids, order, counts, distance bits, or the NaN error, and the nine statistics.

  ("bulk", key, ids, hi, top)   one add_bulk call: ids = a tuple of ids (one id may stand twice: the last vector wins) or ("perm", base, n)
                                = base + a permutation of 0 .. n-1; vector j has 1-24 indices below hi, shuffled, values from a short
                                grid (ties); top (or None) is one further index, above the vocabulary: the row that widens it
  ("empty", id)  ("nan", id)    a row without entries; a row that stores a NaN (payload 0x7fffbeef) at NAN_DIM, which no other row holds
  ("remove", id)  ("flush",)  ("remove_all",)  ("cap", slots)   cap: the workspace lowered to `slots` accumulator slots, 0 restores it
  ("read", key, nq, k, mask, nan)   k an int or ("per", kmax); mask None, ("mask", key) or ("compiled", key); nan: query 0 holds NAN_DIM
  ("reread",)                   the read before, once more: it must equal the model and must not rebuild

THE MODEL is the append log with a live flag per row, answered by spv_data.search_csr; it predicts len, rows, dead_rows, nnz, vocab,
rebuilds, entries_walked, candidates and chunks.  THE REFERENCE ADAPTER (RefIndex) answers another way: the survivors only, as a
fresh dense block, by spv_data.search, each query with its own k.  Its MUTANTS carry one stale-state defect each, modelled on the
engine's state (vdb_spv.cpp); tests/test_spv_lifecycle_cpu.py wants every one caught by a pinned schedule."""
import numpy as np

import spv_data as S

F32, U32, U64 = np.float32, np.uint32, np.uint64
ID_LIMIT = 1 << 14                     # mask bits; ids stay below, but for a few at and above 2^32 that no mask admits
NAN_DIM = 5
GRID = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 1.5, 2.0, 3.0], dtype=F32)
UNTOUCHED_NAN = np.array([0x7fffbeef], dtype=U32).view(F32)[0]
DEFAULT_CAP = 256 << 20
FLOOR = 1024                           # the smallest device array (vdb_spv.cpp upload_tail)


class Predicted(Exception):
    pass


class Mismatch(AssertionError):
    pass


def rng_of(seed, key, salt=0):
    return np.random.default_rng([int(seed), int(key), int(salt)])


def ids_of(seed, key, spec):
    if spec and spec[0] == "perm":
        return (rng_of(seed, key, 1).permutation(spec[2]) + spec[1]).astype(U64)
    return np.array(spec, dtype=U64)


def vectors_of(seed, key, n, hi, top):
    rng = rng_of(seed, key)
    out = []
    for j in range(n):
        idx = np.unique(rng.integers(0, hi, size=rng.integers(1, 25)))
        idx = idx[idx != NAN_DIM]
        if top is not None and j == n - 1:
            idx = np.append(idx, top)
        idx = rng.permutation(idx).astype(U32)
        out.append((idx, GRID[rng.integers(0, GRID.size, idx.size)]))
    return out


def queries_of(seed, key, nq, vocab, nan):
    rng = rng_of(seed, key, 3)
    qs = []
    for b in range(nq):
        idx = np.unique(np.concatenate([rng.integers(0, 8, size=rng.integers(0, 3)), rng.integers(0, vocab + 10, size=rng.integers(1, 12))]))
        idx = idx[idx != NAN_DIM]
        if nan and b == 0:
            idx = np.append(idx, NAN_DIM)
        idx = rng.permutation(idx).astype(U32)
        qs.append((idx, GRID[rng.integers(0, GRID.size, idx.size)]))
    return qs


def ks_of(seed, key, nq, k):
    if isinstance(k, tuple):
        ks = rng_of(seed, key, 4).integers(0, k[1] + 1, size=nq)
        ks[0] = k[1]
        return ks.astype(np.uintp)
    return np.full(nq, k, dtype=np.uintp)


def mask_on(seed, key):
    return rng_of(seed, key, 2).random(ID_LIMIT) < 0.5


def mask_words(on):
    return np.packbits(on.astype(np.uint8), bitorder="little").view(U64)


def chunks_of(nq, cap, n_rows):
    slots = min(nq, max(cap // (4 * n_rows), 1))
    return -(-nq // slots), slots


# ---------------------------------------------------------------------------------------------------------------- the model
class Model:
    def __init__(self):
        self.ids, self.vecs, self.live, self.row_of = [], [], [], {}
        self.nnz = self.vocab = self.rebuilds = 0
        self.dirty, self.cap, self._csr = False, DEFAULT_CAP, None
        self.last = dict(entries_walked=0, candidates=0, chunks=0)
        # what the device arrays hold (capacity in elements, count at the flush before), and what the schedules are asked to cover
        self.cap_rows = self.cap_nnz = 0
        self.flushes, self.first_flush = 0, None
        self.cover = dict(regrow_rows=0, regrow_nnz=0, tail_upload=0, masked_after_regrow=0, masked_after_tail=0, across_1024=0,
                          chunk_change=0, read_empty=0, read_after_remove_all=0, multi_chunk=0, reads=0, nan_reads=0)
        self._since_flush, self._removed_all, self._flush_vocab = None, False, 0

    def bulk(self, ids, vecs):
        for i, v in zip(ids, vecs):
            i = int(i)
            if i in self.row_of:
                self.live[self.row_of[i]] = False
            self.row_of[i] = len(self.ids)
            self.ids.append(i)
            self.vecs.append(v)
            self.live.append(True)
            self.nnz += len(v[0])
            if len(v[0]):
                self.vocab = max(self.vocab, int(max(v[0])) + 1)
        if len(ids):
            self.dirty, self._csr = True, None

    def remove(self, i):
        if int(i) in self.row_of:
            self.live[self.row_of.pop(int(i))] = False
            self.dirty, self._csr = True, None

    def flush(self):
        if not self.dirty:
            return
        self.dirty = False
        self.rebuilds += 1
        rows, nnz = len(self.ids), self.nnz
        grew = []
        if rows + 1 > self.cap_rows:                     # row_ptr holds one more than ids; both regrow together
            grew.append("rows")
            self.cap_rows = max((rows + 1) + (rows + 1) // 2, FLOOR)
        if nnz > self.cap_nnz:
            grew.append("nnz")
            self.cap_nnz = max(nnz + nnz // 2, FLOOR)
        if self.flushes == 0:
            self.first_flush = (rows, nnz)
        else:
            prev_rows, prev_nnz = self._prev
            if "rows" in grew and rows > 1.5 * prev_rows and self.first_flush[0] < FLOOR:
                self.cover["regrow_rows"] += 1
            if "nnz" in grew and nnz > 1.5 * prev_nnz and self.first_flush[1] < FLOOR:
                self.cover["regrow_nnz"] += 1
            if not grew and rows > prev_rows:
                self.cover["tail_upload"] += 1
            self._since_flush = "regrow" if grew else ("tail" if rows > prev_rows else None)
            if self._flush_vocab <= 1024 < self.vocab:
                self.cover["across_1024"] += 1
            if self._flush_vocab and -(-self._flush_vocab // 1024) != -(-self.vocab // 1024):
                self.cover["chunk_change"] += 1
        self._prev, self._flush_vocab = (rows, nnz), self.vocab
        self.flushes += 1

    def csr(self):
        if self._csr is None:
            offsets, indices, values = S.csr_of(self.vecs)
            self._csr = (np.array(self.ids, dtype=U64), offsets, indices, values, np.array(self.live, dtype=bool), S.csc_view(offsets, indices))
        return self._csr

    def stats(self):
        return dict(len=len(self.row_of), rows=len(self.ids), dead_rows=len(self.ids) - len(self.row_of), nnz=self.nnz, vocab=self.vocab,
                    rebuilds=self.rebuilds, **self.last)

    def read(self, queries, ks, on):
        """[(ids, dists), ...] per query, or Predicted; the statistics of the call are in stats() either way"""
        self.flush()
        self.cover["reads"] += 1
        if on is not None and self._since_flush:
            self.cover["masked_after_" + self._since_flush] += 1
            self._since_flush = None
        nq = len(queries)
        self.last = dict(entries_walked=0, candidates=0, chunks=0)
        if not self.row_of:
            self.cover["read_empty"] += 1
        elif self._removed_all:
            self.cover["read_after_remove_all"] += 1
            self._removed_all = False
        if not self.row_of or int(ks.max()) == 0 or not sum(len(q[0]) for q in queries):
            return [(np.zeros(0, U64), np.zeros(0, F32))] * nq
        ids, offsets, indices, values, live, view = self.csr()
        eligible = None
        if on is not None:
            eligible = (ids < ID_LIMIT) & on[np.minimum(ids, ID_LIMIT - 1).astype(np.int64)]
        ctr, out, nan = {}, [], False
        for q, k in zip(queries, ks):
            try:
                out.append(S.search_csr(ids, offsets, indices, values, live, q, int(k), eligible, view, ctr))
            except S.NanScore:
                nan = True
        self.last = dict(entries_walked=ctr["entries_walked"], candidates=ctr["candidates"], chunks=chunks_of(nq, self.cap, len(self.ids))[0])
        if self.last["chunks"] > 1:
            self.cover["multi_chunk"] += 1
        if nan:
            self.cover["nan_reads"] += 1
            raise Predicted("nan")
        return out


# ---------------------------------------------------------------------------------------------------------------- the reference adapter
DEFECTS = ("stale_id_tail", "stale_rank", "dead_row_stays", "readd_first_vector", "vocab_not_widened", "dirty_after_nan",
           "dirty_last_of_chunk", "bulk_keeps_first")


class RefIndex:
    """The survivors only, rebuilt as a fresh dense block per state, answered by the dense spv_data.search.  `defect` makes a mutant."""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect
        self.rows = {}                                   # id -> (row number, indices, values)
        self.n_rows = self.nnz = self.vocab = self.rebuilds = 0
        self.dirty, self.cap, self.block = False, DEFAULT_CAP, None
        self.last = dict(entries_walked=0, candidates=0, chunks=0)
        self.dev_id, self.cap_rows, self.flushed_rows = {}, 0, 0     # the id array as the device holds it, by row number
        self.rank, self.removed_only = None, True
        self.grave, self.built_vocab, self.stale = {}, None, {}
        self.zombies = {}

    def bulk(self, ids, vecs):
        seen = set()
        for i, v in zip(ids, vecs):
            i = int(i)
            self.n_rows += 1
            self.nnz += len(v[0])
            if len(v[0]):
                self.vocab = max(self.vocab, int(max(v[0])) + 1)
            if self.defect == "bulk_keeps_first" and i in seen:
                continue
            seen.add(i)
            if self.defect == "readd_first_vector" and i in self.grave and i not in self.rows:
                v = self.grave[i]
            self.rows[i] = (self.n_rows - 1, v[0], v[1])
        if len(ids):
            self.dirty, self.removed_only = True, False

    def remove(self, i):
        i = int(i)
        if i in self.rows:
            row = self.rows.pop(i)
            self.grave.setdefault(i, (row[1], row[2]))
            if self.defect == "dead_row_stays":
                self.zombies[i] = row
            self.dirty = True

    def __len__(self):
        return len(self.rows)

    def set_cap(self, nbytes):
        self.cap = min(nbytes, DEFAULT_CAP) if nbytes else DEFAULT_CAP

    def flush(self):
        if not self.dirty:
            return
        self.dirty = False
        self.rebuilds += 1
        regrow = self.n_rows + 1 > self.cap_rows
        if regrow:
            self.cap_rows = max((self.n_rows + 1) + (self.n_rows + 1) // 2, FLOOR)
        for i, (r, _, _) in self.rows.items():
            if r >= self.flushed_rows or r not in self.dev_id:
                self.dev_id[r] = 0 if (self.defect == "stale_id_tail" and regrow and self.flushed_rows) else i
        self.flushed_rows = self.n_rows
        if not (self.defect == "stale_rank" and self.removed_only and self.rank is not None):
            self.rank = {i: r for r, i in enumerate(sorted(self.rows))}
        self.sorted = sorted(self.rows)
        self.removed_only = True
        if self.built_vocab is None or self.defect != "vocab_not_widened":
            self.built_vocab = self.vocab
        rows = dict(self.rows)
        rows.update({i: r for i, r in self.zombies.items() if i not in rows})
        order = sorted(rows, key=lambda i: rows[i][0])
        offsets, indices, values = S.csr_of([(rows[i][1], rows[i][2]) for i in order])
        X, P = S.dense_of(offsets, indices, values, max(self.vocab, 1))
        self.block = (np.array(order, dtype=U64), X, P, np.array([self.dev_id.get(rows[i][0], i) for i in order], dtype=U64))

    def stats(self):
        return dict(len=len(self.rows), rows=self.n_rows, dead_rows=self.n_rows - len(self.rows), nnz=self.nnz, vocab=self.vocab,
                    rebuilds=self.rebuilds, **self.last)

    def read(self, queries, ks, on, compiled=False):
        self.flush()
        nq = len(queries)
        self.last = dict(entries_walked=0, candidates=0, chunks=0)
        if not self.rows or int(ks.max()) == 0 or not sum(len(q[0]) for q in queries):
            return [(np.zeros(0, U64), np.zeros(0, F32))] * nq
        ids, X, P, dev = self.block
        eligible = None
        if on is not None:
            eligible = (dev < ID_LIMIT) & on[np.minimum(dev, ID_LIMIT - 1).astype(np.int64)]
        chunks, slots = chunks_of(nq, self.cap, self.n_rows)
        self.last["chunks"] = chunks
        out, nan = [], False
        for b, (q, k) in enumerate(zip(queries, ks)):
            keep = np.asarray(q[0]) < self.built_vocab
            q = (np.asarray(q[0])[keep], np.asarray(q[1])[keep])
            touched, s = S.scores(X, P, q)
            self.last["entries_walked"] += int(P[:, q[0][q[0] < P.shape[1]]].sum())
            stale = self.stale.pop(b % slots, None)
            if stale is not None:                        # (mutants only) the fold starts from what the slot was left with
                at = {int(i): r for r, i in enumerate(ids)}
                for i, v in stale:
                    if i in at and touched[at[i]]:
                        with np.errstate(all="ignore"):
                            X2 = v + s[at[i]]
                        s[at[i]] = X2
            cand = touched if eligible is None else touched & eligible
            self.last["candidates"] += int(cand.sum())
            rows = np.flatnonzero(cand)
            bad = bool(np.isnan(s[rows]).any())
            nan |= bad
            if (self.defect == "dirty_after_nan" and bad) or (self.defect == "dirty_last_of_chunk" and (b % slots == slots - 1 or b == nq - 1)):
                self.stale[b % slots] = [(int(i), v) for i, v in zip(ids[touched], s[touched])]
            if not bad:
                d = -s[rows]
                o = np.lexsort((ids[rows], S.ordered(d)))[:int(k)]
                got = ids[rows][o]
                if self.defect == "stale_rank":          # out id = sorted ids [rank of the row]
                    got = np.array([self.sorted[min(self.rank.get(int(i), 0), len(self.sorted) - 1)] for i in got], dtype=U64)
                out.append((got, d[o]))
        if nan:
            raise Predicted("nan")
        return out


# ---------------------------------------------------------------------------------------------------------------- the runner
def run(trace, adapter, model=None):
    """every op to the adapter and to the model; Mismatch names the op.  Returns the model (its .cover counts the edges met)."""
    seed, m = trace["seed"], model or Model()
    last_read = None
    for n, op in enumerate(trace["ops"]):
        kind = op[0]
        if kind == "reread":
            op, kind, again = last_read, "read", True
        else:
            again = False
        if kind == "bulk":
            ids = ids_of(seed, op[1], op[2])
            vecs = vectors_of(seed, op[1], ids.size, op[3], op[4])
            m.bulk(ids, vecs)
            adapter.bulk(ids, vecs)
        elif kind == "empty":
            for x in (m, adapter):
                x.bulk(np.array([op[1]], U64), [(np.zeros(0, U32), np.zeros(0, F32))])
        elif kind == "nan":
            for x in (m, adapter):
                x.bulk(np.array([op[1]], U64), [(np.array([NAN_DIM], U32), np.array([UNTOUCHED_NAN], F32))])
        elif kind == "remove":
            m.remove(op[1])
            adapter.remove(op[1])
        elif kind == "remove_all":
            for i in list(m.row_of):
                m.remove(i)
                adapter.remove(i)
            m._removed_all = True
        elif kind == "flush":
            m.flush()
            adapter.flush()
        elif kind == "cap":
            nbytes = 4 * len(m.ids) * op[1]              # (0 restores the default, as it does in the engine)
            m.cap = min(nbytes, DEFAULT_CAP) if nbytes else DEFAULT_CAP
            adapter.set_cap(nbytes)
        elif kind == "read":
            last_read = op
            _, key, nq, k, mask, nan = op
            queries, ks = queries_of(seed, key, nq, m.vocab, nan), ks_of(seed, key, nq, k)
            on = mask_on(seed, mask[1]) if mask else None
            rebuilds = m.rebuilds
            try:
                want = m.read(queries, ks, on)
            except Predicted:
                want = None
            if again and m.rebuilds != rebuilds:
                raise Mismatch("op %d: the model rebuilt on a reread" % n)
            try:
                got = adapter.read(queries, ks, on, compiled=bool(mask and mask[0] == "compiled"))
            except Predicted:
                got = None
            where = "op %d %r" % (n, op)
            if (got is None) != (want is None):
                raise Mismatch("%s: NaN error %s, the model %s" % (where, got is None, want is None))
            for b in range(nq if want is not None else 0):
                if not (np.array_equal(got[b][0], want[b][0]) and np.array_equal(got[b][1].view(U32), want[b][1].view(U32))):
                    raise Mismatch("%s: query %d differs: %r / %r" % (where, b, got[b][0][:8], want[b][0][:8]))
            gs, ws = adapter.stats(), m.stats()
            if gs != ws:
                raise Mismatch("%s: statistics %r, the model %r" % (where, gs, ws))
        else:
            raise ValueError(op)
        if len(adapter) != len(m.row_of):
            raise Mismatch("op %d %r: len %d, the model %d" % (n, op, len(adapter), len(m.row_of)))
    return m


# ---------------------------------------------------------------------------------------------------------------- the schedules
class _Gen:
    """deals one schedule: a small first flush, then mutations and reads by weight, with the segments a profile asks for"""

    def __init__(self, seed, n_ops, profile):
        self.rng, self.seed, self.ops, self.key = np.random.default_rng([20420, seed]), seed, [], 0
        self.alive, self.dead, self.next_id, self.vocab, self.n_rows = [], [], 10, 0, 0
        self.profile, self.n_ops = profile, n_ops

    def k(self):
        self.key += 1
        return self.key

    def fresh(self, n):
        base = self.next_id
        self.next_id += n
        return base

    def bulk(self, n, hi=None, top=None, ids=None):
        hi = hi or max(self.vocab, 40)
        if ids is None:
            base = self.fresh(n)
            spec = ("perm", base, n) if n > 3 else tuple(range(base, base + n))
            new = list(range(base, base + n))
        else:
            spec, new = tuple(ids), list(dict.fromkeys(ids))
        self.ops.append(("bulk", self.k(), spec, hi, top))
        self.alive = [i for i in self.alive if i not in set(new)] + new
        self.dead = [i for i in self.dead if i not in set(new)]
        self.vocab = max(self.vocab, hi if top is None else top + 1)
        self.n_rows += len(spec) if ids is not None else n

    def read(self, nq=None, k=None, mask=None, nan=False):
        rng = self.rng
        nq = nq or int(rng.choice([1, 1, 3, 8]))
        k = k if k is not None else [1, 10, 100, 1024, ("per", 64), ("per", 1024)][rng.integers(0, 6)]
        self.ops.append(("read", self.k(), nq, k, mask, nan))

    def masked(self):
        self.read(mask=(("mask", "compiled")[self.rng.integers(0, 2)], self.k()))

    def step(self):
        rng, r = self.rng, self.rng.random()
        if r < 0.10:
            self.bulk(1)
        elif r < 0.20:
            self.bulk(int(rng.choice([2, 7, 60, 300])))
        elif r < 0.28 and self.alive:
            a = int(rng.choice(self.alive))
            self.bulk(0, ids=[a, int(rng.choice(self.alive)), a] if rng.random() < 0.5 else [a])
        elif r < 0.38 and self.alive:
            i = self.alive.pop(int(rng.integers(0, len(self.alive))))
            self.dead.append(i)
            self.ops.append(("remove", i))
        elif r < 0.41:
            self.ops.append(("remove", 9_000_000 + int(rng.integers(0, 100))))
        elif r < 0.47 and self.dead:
            self.bulk(0, ids=[int(rng.choice(self.dead))])
        elif r < 0.50:
            i = self.fresh(1)
            self.ops.append(("empty", i))
            self.alive.append(i)
            self.n_rows += 1
        elif r < 0.53:
            self.ops.append(("flush",))
        elif r < 0.56:
            big = (1 << 32) + int(rng.integers(0, 50))
            self.bulk(0, ids=[big])
        elif r < 0.70:
            self.masked()
        elif r < 0.74:
            self.read()
            self.ops.append(("reread",))
        else:
            self.read()

    def deal(self):
        p = self.profile
        self.bulk(int(self.rng.integers(5, 40)), hi=40)                 # the first flush: far below the allocation floor
        self.read()
        for _ in range(self.n_ops // 3):
            self.step()
        if p == "regrow":                                # rows and entries past 1.5 x the floor in one flush, then a pure tail
            self.ops.append(("flush",))
            self.bulk(int(self.rng.integers(1700, 2600)))
            self.masked()
            self.bulk(int(self.rng.integers(5, 40)))
            self.ops.append(("flush",))
            self.masked()
        elif p == "widen":                               # across 1024 in one step, then past the scan's next chunk sizes
            for top in (int(self.rng.integers(1024, 1100)), 2047, 2048, int(self.rng.integers(3073, 3300))):
                self.bulk(1, top=top)
                self.read(nq=3)
                self.masked()
        elif p == "empty":                               # nothing alive, then a new life
            self.ops.append(("remove_all",))
            self.alive, self.dead = [], self.dead + self.alive
            self.read()
            self.masked()
            self.bulk(int(self.rng.integers(20, 200)))
            self.read()
            self.ops.append(("reread",))
        elif p == "nan":                                 # a stored NaN: an error while it is eligible, and a clean slot after it
            i = self.fresh(1)
            self.ops.append(("nan", i))
            self.n_rows += 1
            self.read(nq=3, k=10, nan=True)
            self.read(nq=3, k=10)
            self.ops.append(("reread",))
            self.ops.append(("remove", i))
            self.read(nq=2, k=10, nan=True)
        elif p == "chunks":                              # a low cap: batches of several chunks, the last slot reused
            self.ops.append(("cap", 3))
            self.read(nq=8)
            self.ops.append(("reread",))
            self.read(nq=7, k=10)
            self.masked()
            self.ops.append(("cap", 0))
            self.read(nq=8)
        while len(self.ops) < self.n_ops:
            self.step()
        self.read(nq=3, k=1024)
        self.ops.append(("reread",))
        return {"seed": self.seed, "ops": self.ops}


PROFILES = ("regrow", "widen", "empty", "nan", "chunks", "regrow", "widen", "empty", "nan", "chunks", "regrow", "widen")
_PINNED = None


def pinned():
    """the dozen pinned schedules, 40-80 ops each; dealt once"""
    global _PINNED
    if _PINNED is None:
        _PINNED = [_Gen(100 + j, 40 + 3 * j, p).deal() for j, p in enumerate(PROFILES)]
    return _PINNED

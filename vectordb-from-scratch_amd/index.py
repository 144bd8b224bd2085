"""Host-side mirror of the reference's `Index` trait (src/index.rs:11-35) and the GPU-backed
implementation that replaces `FlatIndex` (src/flat_index.rs:12-74) behind it.

`GpuFlatIndex` owns ids and a host copy of each row (the trait's `get_vector` returns a
borrow, so the host keeps one anyway) and calls the hand-written HIP kernels through the C
ABI of include/vdb_flat.h.  There is no CPU search path."""
import abc
import ctypes
import os

import numpy as np

from . import _ffi
from .error import DimensionMismatch, IndexError_, InvalidVector, NanDistance, VectorNotFound
from .vector import DistanceMetric, Vector


def _raise(rc):
    msg, exp, act = _ffi.last_error()
    if rc == _ffi.ERR_DIMENSION_MISMATCH:
        raise DimensionMismatch(exp, act)
    if rc == _ffi.ERR_INVALID_VECTOR:
        raise InvalidVector(msg.split(": ", 1)[-1])
    if rc == _ffi.ERR_NAN:
        raise NanDistance(msg)
    raise IndexError_(msg)


class Index(abc.ABC):
    """trait Index  (src/index.rs:11-35)"""

    @abc.abstractmethod
    def add(self, id, vector): ...

    @abc.abstractmethod
    def remove(self, id): ...

    @abc.abstractmethod
    def search(self, query, k): ...

    @abc.abstractmethod
    def get_vector(self, id): ...

    @abc.abstractmethod
    def metric(self): ...

    @abc.abstractmethod
    def len(self): ...

    def is_empty(self):                              # index.rs:32-34
        return self.len() == 0

    def search_batch(self, queries):
        """The provided method SURVEY.md 8(b) proposes adding to the trait: default = the
        sequential loop of VectorStore::search_batch (storage.rs:306-309)."""
        return [self.search(q, k) for q, k in queries]

    def __len__(self):
        return self.len()


def _fp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _u64p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))


class CompiledMask:
    """A filter compiled on the device (MetaTable.compile): the id bitmask in HBM plus the event behind which it is complete.
    release() gives the buffer back to the table's pool -- after the last search that reads the mask has completed."""

    def __init__(self, table, handle):
        self._table, self._m = table, handle             # (the table is kept alive: it owns the buffer)

    @property
    def handle(self):
        if not self._m:
            raise ValueError("the compiled mask was released")
        if not self._table._t:                           # (a closed table has freed every mask it handed out)
            raise ValueError("the compiled mask's table was closed")
        return self._m

    @property
    def ptr(self):
        """device pointer of the mask words, for the mask_ptr of the search_batch_device* calls (after wait_on)"""
        return int(self._table._L.vdb_meta_mask_ptr(self.handle) or 0)

    @property
    def bits(self):
        return int(self._table._L.vdb_meta_mask_bits(self.handle))

    def count(self):
        """eligible ids (set bits); waits for the compile"""
        n = ctypes.c_uint64(0)
        rc = self._table._L.vdb_meta_mask_count(self.handle, ctypes.byref(n))
        if rc:
            _raise(rc)
        return int(n.value)

    def wait_on(self, stream=0):
        """order `stream` (a hipStream_t as an integer, 0 = the null stream) behind the mask; the host does not wait"""
        rc = self._table._L.vdb_meta_mask_wait_on(self.handle, ctypes.c_void_p(stream or None))
        if rc:
            _raise(rc)

    def release(self):
        m, self._m = self._m, None
        if m and self._table._t:
            rc = self._table._L.vdb_meta_mask_release(m)
            if rc:
                _raise(rc)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()


class MetaTable:
    """The store's metadata resident on one GPU (include/vdb_flat.h vdb_meta_table): int32 dictionary-code columns by slot
    and a presence bitmap, both by internal id.  Writes are staged and uploaded by the next compile()."""

    EQ, NE, EXISTS, CONST, AND, OR = range(6)
    LT, LE, GT, GE = 16, 17, 18, 19
    MAX_OPS, MAX_DEPTH, MAX_CONSTS = 1024, 32, 1024

    def __init__(self, device=0):
        self._L = _ffi.lib()
        self._t = ctypes.c_void_p()
        rc = self._L.vdb_meta_create(int(device), ctypes.byref(self._t))
        if rc:
            _raise(rc)
        self.device = int(device)

    def close(self):
        t, self._t = getattr(self, "_t", None), None
        if t:
            self._L.vdb_meta_destroy(t)

    __del__ = close

    def set_codes(self, slot, first_id, codes):
        c = np.ascontiguousarray(codes, dtype=np.int32)
        rc = self._L.vdb_meta_set_codes(self._t, int(slot), int(first_id), c.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), c.size)
        if rc:
            _raise(rc)

    def set_present(self, first_id, n, on):
        rc = self._L.vdb_meta_set_present(self._t, int(first_id), int(n), 1 if on else 0)
        if rc:
            _raise(rc)

    def set_numbers(self, slot, first_code, values):
        """The numeric LUT of column `slot`: values[i] is the number of dictionary code first_code + i, NaN = the code's string
        has no number (vdb_meta_set_numbers).  What LT / LE / GT / GE leaves on that column compare."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        if not 0 <= int(first_code) < 1 << 32:
            raise ValueError("first_code must fit 32 bits")
        rc = self._L.vdb_meta_set_numbers(self._t, int(slot), int(first_code), v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), v.size)
        if rc:
            _raise(rc)

    def compile(self, program, mask_bits, consts=None):
        """program: a sequence of (op, slot, code) in postfix order; consts: the f64 constants its LT / LE / GT / GE leaves
        index with `code` (None: vdb_meta_compile, which refuses such leaves).  Returns a CompiledMask without waiting for the
        device."""
        ops = (_ffi.MetaOp * max(len(program), 1))()
        for i, (op, slot, code) in enumerate(program):
            ops[i].op, ops[i].slot, ops[i].code = int(op), int(slot), int(code)
        m = ctypes.c_void_p()
        if consts is None:
            rc = self._L.vdb_meta_compile(self._t, ops, len(program), int(mask_bits), ctypes.byref(m))
        else:
            cs = np.ascontiguousarray(consts, dtype=np.float64)
            rc = self._L.vdb_meta_compile_num(self._t, ops, len(program), cs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), cs.size,
                                              int(mask_bits), ctypes.byref(m))
        if rc:
            _raise(rc)
        return CompiledMask(self, m)


GROUP_NONE = 0xFFFFFFFF                              # search_batch_grouped: this query is searched without a filter


class GpuFlatIndex(Index):
    """Drop-in for FlatIndex (src/flat_index.rs) backed by the MI355X engine."""

    EXCHANGE_RCCL, EXCHANGE_PEER = 0, 1
    GROUP_NONE = GROUP_NONE                              # search_batch_grouped: this query is searched without a filter

    def __init__(self, metric, device=0, keep_host_copy=True, devices=None):
        """devices=[d0, d1, ...]: ONE index whose rows are sharded over these GPUs inside this process
        (vdb_flat_create_sharded; queries and outputs live on d0).  Every method below works on it unchanged."""
        self._metric = DistanceMetric(metric)
        self._h = ctypes.c_void_p()
        self._L = _ffi.lib()
        if devices is not None:
            devs = (ctypes.c_int * len(devices))(*[int(d) for d in devices])
            rc = self._L.vdb_flat_create_sharded(int(self._metric), devs, len(devices), ctypes.byref(self._h))
            device = devices[0] if len(devices) else 0
        else:
            rc = self._L.vdb_flat_create(int(self._metric), int(device), ctypes.byref(self._h))
        if rc:
            _raise(rc)
        self._device = int(device)
        self._keep = keep_host_copy
        self._vectors = {}                           # id -> Vector (for get_vector borrows)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.vdb_flat_destroy(h)

    # ---- Index trait
    def add(self, id, vector):                       # flat_index.rs:38-41
        v = vector if isinstance(vector, Vector) else Vector(vector)
        rc = self._L.vdb_flat_add(self._h, int(id), _fp(v.data), v.dimension())
        if rc:
            _raise(rc)
        if self._keep:
            self._vectors[int(id)] = v

    def remove(self, id):                            # flat_index.rs:43-46
        rc = self._L.vdb_flat_remove(self._h, int(id))
        if rc:
            _raise(rc)
        self._vectors.pop(int(id), None)

    def get_vector(self, id):                        # flat_index.rs:48-50
        if self._keep:
            return self._vectors.get(int(id))
        dim = ctypes.c_size_t()
        rc = self._L.vdb_flat_get_vector(self._h, int(id), None, 0, ctypes.byref(dim))
        if rc == _ffi.ERR_NOT_FOUND:
            return None
        if rc:
            _raise(rc)
        out = np.zeros(dim.value, dtype=np.float32)
        rc = self._L.vdb_flat_get_vector(self._h, int(id), _fp(out), out.size, ctypes.byref(dim))
        if rc:
            _raise(rc)
        return Vector(out)

    def search(self, query, k):                      # flat_index.rs:52-65
        q = query if isinstance(query, Vector) else Vector(query)
        res = self.search_batch([(q, k)])
        return res[0]

    def metric(self):                                # flat_index.rs:67-69
        return self._metric

    def len(self):                                   # flat_index.rs:71-73
        return int(self._L.vdb_flat_len(self._h))

    # ---- batched hot call (overrides the provided loop)
    def search_batch(self, queries, id_mask=None, mask_bits=0, compiled_mask=None):
        """queries: sequence of (Vector, k).  Returns a list of [(id, distance), ...] per query.
        compiled_mask: a CompiledMask (MetaTable.compile) instead of id_mask / mask_bits; results are identical."""
        if len(queries) == 0:
            return []
        dims = {q.dimension() for q, _ in queries}
        if len(dims) != 1:
            # a ragged batch: the reference handles each query on its own (storage.rs:306-309)
            return [self.search_batch([(q, k)], id_mask, mask_bits, compiled_mask)[0] for q, k in queries]
        qs = np.stack([q.data for q, _ in queries]).astype(np.float32, copy=False)
        ks = np.array([int(k) for _, k in queries], dtype=np.uintp)
        ids, dists, counts = self.search_batch_arrays(qs, ks, id_mask=id_mask, mask_bits=mask_bits, compiled_mask=compiled_mask)
        return [[(int(ids[b, i]), np.float32(dists[b, i])) for i in range(int(counts[b]))] for b in range(len(queries))]

    def search_batch_arrays(self, queries, k, id_mask=None, mask_bits=0, compiled_mask=None):
        """numpy in/out form: queries [nq, dim] f32, k an int or a per-query array.
        Returns (ids u64 [nq,kmax], dists f32 [nq,kmax], counts [nq])."""
        if compiled_mask is not None and id_mask is not None:
            raise ValueError("pass id_mask or compiled_mask, not both")
        qs = np.ascontiguousarray(queries, dtype=np.float32)
        nq, dim = qs.shape
        if np.isscalar(k):
            ks_ptr, kscalar, kmax = None, int(k), int(k)
        else:
            ks = np.ascontiguousarray(k, dtype=np.uintp)
            ks_ptr = ks.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
            kscalar, kmax = 0, int(ks.max()) if ks.size else 0
        kstride = max(kmax, 1)
        out_ids = np.zeros((nq, kstride), dtype=np.uint64)
        out_d = np.zeros((nq, kstride), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uintp)
        mask_ptr = None
        if id_mask is not None:
            m = np.ascontiguousarray(id_mask, dtype=np.uint64)
            mask_ptr = _u64p(m)
        if compiled_mask is not None:
            rc = self._L.vdb_flat_search_batch_filtered(self._h, _fp(qs), nq, dim, ks_ptr, kscalar, compiled_mask.handle,
                                                        kstride, _u64p(out_ids), _fp(out_d),
                                                        counts.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)))
        else:
            rc = self._L.vdb_flat_search_batch(self._h, _fp(qs), nq, dim, ks_ptr, kscalar, mask_ptr, int(mask_bits),
                                               kstride, _u64p(out_ids), _fp(out_d),
                                               counts.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)))
        if rc:
            _raise(rc)
        return out_ids, out_d, counts

    # ---- search by stored id (include/vdb_flat.h vdb_flat_search_batch_by_id; no reference counterpart)
    def search_batch_by_id(self, ids, k, id_mask=None, mask_bits=0, compiled_mask=None):
        """The nearest neighbours of STORED vectors, the vector itself left out: for query id x, what search_batch_arrays
        returns for the stored vector of x with k + 1, the entry whose id equals x removed if it is there, cut to k.  The
        vectors never leave the device.  ids: u64 array of stored ids (repeats allowed); k an int or a per-query array.
        Returns the arrays of search_batch_arrays.  An id that is not stored raises VectorNotFound for the whole batch."""
        if compiled_mask is not None and id_mask is not None:
            raise ValueError("pass id_mask or compiled_mask, not both")
        qid = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        nq = qid.size
        if np.isscalar(k):
            ks_ptr, kscalar, kmax = None, int(k), int(k)
        else:
            ks = np.ascontiguousarray(k, dtype=np.uintp)
            if ks.shape != (nq,):
                raise ValueError(f"k must be a scalar or hold one value per query id ({nq}), not {ks.shape}")
            ks_ptr = ks.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
            kscalar, kmax = 0, int(ks.max()) if ks.size else 0
        kstride = max(kmax, 1)
        out_ids = np.zeros((nq, kstride), dtype=np.uint64)
        out_d = np.zeros((nq, kstride), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uintp)
        cp = counts.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
        if compiled_mask is not None:
            rc = self._L.vdb_flat_search_batch_by_id_filtered(self._h, _u64p(qid), nq, ks_ptr, kscalar, compiled_mask.handle,
                                                              kstride, _u64p(out_ids), _fp(out_d), cp)
        else:
            mask_ptr = None
            if id_mask is not None:
                m = np.ascontiguousarray(id_mask, dtype=np.uint64)
                mask_ptr = _u64p(m)
            rc = self._L.vdb_flat_search_batch_by_id(self._h, _u64p(qid), nq, ks_ptr, kscalar, mask_ptr, int(mask_bits),
                                                     kstride, _u64p(out_ids), _fp(out_d), cp)
        if rc == _ffi.ERR_NOT_FOUND:
            raise VectorNotFound(int(_ffi.last_error()[0].rsplit(": ", 1)[-1]))
        if rc:
            _raise(rc)
        return out_ids, out_d, counts

    def by_id_stats(self):
        """The last search_batch_by_id: [0] queries, [1] queries whose own id was found in their list and struck, [2] queries
        whose list was cut instead, [3] 0.  The lists are those the device searched: max(k) + 1 entries for every query, so with a
        per-query k a query counts as struck when its own id lies anywhere among its max(k) + 1 nearest."""
        out = (ctypes.c_uint64 * 4)()
        rc = self._L.vdb_flat_by_id_stats(self._h, out)
        if rc:
            _raise(rc)
        return [int(x) for x in out]

    def _recommend(self, best, positive, negative, k, id_mask, mask_bits, compiled_mask):
        """what recommend_batch and recommend_best_batch share: the example lists as the C ABI takes them, the outputs (with the
        negatives' distances for `best`), the call under either kind of mask, the errors"""
        if compiled_mask is not None and id_mask is not None:
            raise ValueError("pass id_mask or compiled_mask, not both")
        nq = len(positive)
        if negative is None:
            negative = [()] * nq
        if len(negative) != nq:
            raise ValueError(f"{nq} positive lists but {len(negative)} negative lists")
        pos = [np.asarray(p, dtype=np.uint64).reshape(-1) for p in positive]
        neg = [np.asarray(x, dtype=np.uint64).reshape(-1) for x in negative]
        ex = np.ascontiguousarray(np.concatenate([a for pn in zip(pos, neg) for a in pn] + [np.zeros(0, dtype=np.uint64)]))
        offsets = np.zeros(nq + 1, dtype=np.uintp)
        offsets[1:] = np.cumsum([p.size + x.size for p, x in zip(pos, neg)], dtype=np.uintp)
        n_pos = np.asarray([p.size for p in pos], dtype=np.uint32)
        if np.isscalar(k):
            ks_ptr, kscalar, kmax = None, int(k), int(k)
        else:
            ks = np.ascontiguousarray(k, dtype=np.uintp)
            if ks.shape != (nq,):
                raise ValueError(f"k must be a scalar or hold one value per request ({nq}), not {ks.shape}")
            ks_ptr = ks.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
            kscalar, kmax = 0, int(ks.max()) if ks.size else 0
        kstride = max(kmax, 1)
        out_ids = np.zeros((nq, kstride), dtype=np.uint64)
        out_d = np.zeros((nq, kstride), dtype=np.float32)
        out_n = np.zeros((nq, kstride), dtype=np.float32) if best else None
        counts = np.zeros(nq, dtype=np.uintp)
        szp = ctypes.POINTER(ctypes.c_size_t)
        head = (self._h, _u64p(ex), offsets.ctypes.data_as(szp), n_pos.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), nq, ks_ptr, kscalar)
        tail = (kstride, _u64p(out_ids), _fp(out_d)) + ((_fp(out_n),) if best else ()) + (counts.ctypes.data_as(szp),)
        plain, filtered = ((self._L.vdb_flat_recommend_best_batch, self._L.vdb_flat_recommend_best_batch_filtered) if best else
                           (self._L.vdb_flat_recommend_batch, self._L.vdb_flat_recommend_batch_filtered))
        if compiled_mask is not None:
            rc = filtered(*head, compiled_mask.handle, *tail)
        else:
            mask_ptr = None
            if id_mask is not None:
                m = np.ascontiguousarray(id_mask, dtype=np.uint64)
                mask_ptr = _u64p(m)
            rc = plain(*head, mask_ptr, int(mask_bits), *tail)
        if rc == _ffi.ERR_NOT_FOUND:
            raise VectorNotFound(int(_ffi.last_error()[0].rsplit(": ", 1)[-1]))
        if rc:
            _raise(rc)
        return (out_ids, out_d, out_n, counts) if best else (out_ids, out_d, counts)

    # ---- recommend from positive and negative stored ids (include/vdb_flat.h vdb_flat_recommend_batch; no reference counterpart)
    def recommend_batch(self, positive, negative, k, id_mask=None, mask_bits=0, compiled_mask=None):
        """"More like these, less like those": request b is the average ap of the stored vectors positive[b] (at least one id)
        and, when negative[b] is not empty, ap + (ap - an) with the average an of those; the answer is what
        search_batch_arrays returns for that vector with k + the number of examples, every example removed, cut to k.  The
        fold runs on the device in f32, left to right in list order (include/vdb_flat.h has the exact arithmetic); the
        vectors never leave it.  positive, negative: sequences of id sequences of the same length (negative None: no
        negatives at all); k an int or a per-request array.  Returns the arrays of search_batch_arrays.  An id that is not
        stored raises VectorNotFound for the whole batch."""
        return self._recommend(False, positive, negative, k, id_mask, mask_bits, compiled_mask)

    def recommend_stats(self):
        """The last recommend_batch: [0] requests, [1] example rows folded, [2] entries struck in total (those in front of the
        cut of the batch-wide list), [3] the depth the search ran at: min(max(k), len) + the longest request, at most len."""
        out = (ctypes.c_uint64 * 4)()
        rc = self._L.vdb_flat_recommend_stats(self._h, out)
        if rc:
            _raise(rc)
        return [int(x) for x in out]

    # ---- recommend by best score (include/vdb_flat.h vdb_flat_recommend_best_batch; no reference counterpart)
    def recommend_best_batch(self, positive, negative, k, id_mask=None, mask_bits=0, compiled_mask=None):
        """Nearest to ANY positive, vetoed by the negatives: every candidate row x is scored against every example on its own.
        dp(x) is the smallest distance from a positive of the request to x (the distance search_batch_by_id reports), x is kept
        when dp(x) is strictly below its distance from every negative, and the answer is the kept rows nearest first by
        (dp, id), the examples themselves left out (include/vdb_flat.h has the exact rules).  positive, negative, k and the
        masks as in recommend_batch.  Returns (ids u64 [nq, kmax], dists f32 [nq, kmax] -- dp --, neg_dists f32 [nq, kmax] --
        the smallest distance from a negative, +inf without negatives --, counts [nq]).  An id that is not stored raises
        VectorNotFound for the whole batch."""
        return self._recommend(True, positive, negative, k, id_mask, mask_bits, compiled_mask)

    def recommend_best_stats(self):
        """The last recommend_best_batch: [0] requests, [1] example rows, [2] requests answered at list stage 0, [3] at list
        stage 1, [4] by the exact scan, [5] the stage-0 depth, [6] list searches run (the positives of every stage a request
        went through), [7] 0."""
        out = (ctypes.c_uint64 * 8)()
        rc = self._L.vdb_flat_recommend_best_stats(self._h, out)
        if rc:
            _raise(rc)
        return [int(x) for x in out]

    def debug_set_recommend_best_route(self, mode):
        """Tests: 0 automatic, 1 the list stages first whatever the depth, 2 the exact scan only.  The answers are the same bits."""
        rc = self._L.vdb_flat_debug_set_recommend_best_route(self._h, int(mode))
        if rc:
            _raise(rc)

    # ---- discovery search (include/vdb_flat.h vdb_flat_discover_batch; no reference counterpart)
    def discover_batch(self, targets, pairs, k, id_mask=None, mask_bits=0, compiled_mask=None, want_ranks=True):
        """A target ranked inside context pairs: request b has the stored id targets[b] and the (positive id, negative id) pairs
        pairs[b] (at most 16, may be empty).  rank(x) counts the pairs whose positive is strictly nearer to row x than their
        negative (the distances search_batch_by_id reports), and the answer is the rows by (rank descending, distance from the
        target ascending, id), the target and every pair id left out (include/vdb_flat.h has the exact rules).  k an int or a
        per-request array; the masks as in recommend_batch.  Returns (ids u64 [nq, kmax], dists f32 [nq, kmax] -- from the
        target --, ranks u32 [nq, kmax] or None without want_ranks, counts [nq]).  An id that is not stored raises VectorNotFound
        for the whole batch."""
        if compiled_mask is not None and id_mask is not None:
            raise ValueError("pass id_mask or compiled_mask, not both")
        tg = np.ascontiguousarray(targets, dtype=np.uint64).reshape(-1)
        nq = tg.size
        if len(pairs) != nq:
            raise ValueError(f"{nq} targets but {len(pairs)} pair lists")
        pl = [np.asarray(p, dtype=np.uint64).reshape(-1, 2) for p in pairs]
        flat = np.ascontiguousarray(np.concatenate([p.reshape(-1) for p in pl] + [np.zeros(0, dtype=np.uint64)]))
        offsets = np.zeros(nq + 1, dtype=np.uintp)
        offsets[1:] = np.cumsum([p.shape[0] for p in pl], dtype=np.uintp)
        if np.isscalar(k):
            ks_ptr, kscalar, kmax = None, int(k), int(k)
        else:
            ks = np.ascontiguousarray(k, dtype=np.uintp)
            if ks.shape != (nq,):
                raise ValueError(f"k must be a scalar or hold one value per request ({nq}), not {ks.shape}")
            ks_ptr = ks.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
            kscalar, kmax = 0, int(ks.max()) if ks.size else 0
        kstride = max(kmax, 1)
        out_ids = np.zeros((nq, kstride), dtype=np.uint64)
        out_d = np.zeros((nq, kstride), dtype=np.float32)
        out_r = np.zeros((nq, kstride), dtype=np.uint32) if want_ranks else None
        counts = np.zeros(nq, dtype=np.uintp)
        szp = ctypes.POINTER(ctypes.c_size_t)
        head = (self._h, _u64p(tg), _u64p(flat), offsets.ctypes.data_as(szp), nq, ks_ptr, kscalar)
        tail = (kstride, _u64p(out_ids), _fp(out_d), out_r.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if want_ranks else None,
                counts.ctypes.data_as(szp))
        if compiled_mask is not None:
            rc = self._L.vdb_flat_discover_batch_filtered(*head, compiled_mask.handle, *tail)
        else:
            mask_ptr = None
            if id_mask is not None:
                m = np.ascontiguousarray(id_mask, dtype=np.uint64)
                mask_ptr = _u64p(m)
            rc = self._L.vdb_flat_discover_batch(*head, mask_ptr, int(mask_bits), *tail)
        if rc == _ffi.ERR_NOT_FOUND:
            raise VectorNotFound(int(_ffi.last_error()[0].rsplit(": ", 1)[-1]))
        if rc:
            _raise(rc)
        return out_ids, out_d, out_r, counts

    def discover_stats(self):
        """The last discover_batch: [0] requests, [1] example rows (targets included), [2] requests answered at list stage 0,
        [3] at list stage 1, [4] by the exact scan, [5] the stage-0 depth, [6] list searches run (one per request and stage it
        went through), [7] 0."""
        out = (ctypes.c_uint64 * 8)()
        rc = self._L.vdb_flat_discover_stats(self._h, out)
        if rc:
            _raise(rc)
        return [int(x) for x in out]

    def debug_set_discover_route(self, mode):
        """Tests: 0 automatic, 1 the list stages first whatever the depth, 2 the exact scan only.  The answers are the same bits."""
        rc = self._L.vdb_flat_debug_set_discover_route(self._h, int(mode))
        if rc:
            _raise(rc)

    # ---- diverse top-k, MMR on the device (include/vdb_flat.h vdb_flat_search_batch_mmr; no reference counterpart)
    def search_batch_mmr(self, queries, k, candidates, lam, id_mask=None, mask_bits=0, compiled_mask=None, ks=None):
        """k results that are not all the same thing: the `candidates` nearest rows of each query (what search_batch_arrays
        returns at that depth) are re-ranked greedily on the device -- pick 1 is the nearest, every later pick minimises
        lam * d - (1 - lam) * (distance to the nearest row already picked), ties by position in the candidate list
        (include/vdb_flat.h has the exact arithmetic).  lam is a scalar or one value per query, within [0, 1]; lam = 1 is the
        plain search.  ks: one k per query instead of k.  1 <= k <= candidates <= 1024.  Returns (ids u64 [nq, kmax],
        dists f32 [nq, kmax] -- the query distance of each pick --, scores f32 [nq, kmax], counts [nq]), in pick order."""
        if compiled_mask is not None and id_mask is not None:
            raise ValueError("pass id_mask or compiled_mask, not both")
        qs = np.ascontiguousarray(queries, dtype=np.float32)
        nq, dim = qs.shape
        if ks is None:
            ks_ptr, kscalar, kmax = None, int(k), int(k)
        else:
            ksa = np.ascontiguousarray(ks, dtype=np.uintp)
            if ksa.shape != (nq,):
                raise ValueError(f"ks must hold one value per query ({nq}), not {ksa.shape}")
            ks_ptr = ksa.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
            kscalar, kmax = 0, int(ksa.max()) if ksa.size else 0
        if np.isscalar(lam):
            lam_ptr, lscalar = None, float(lam)
        else:
            lams = np.ascontiguousarray(lam, dtype=np.float32)
            if lams.shape != (nq,):
                raise ValueError(f"lam must be a scalar or hold one value per query ({nq}), not {lams.shape}")
            lam_ptr, lscalar = _fp(lams), 0.0
        kstride = max(kmax, 1)
        out_ids = np.zeros((nq, kstride), dtype=np.uint64)
        out_d = np.zeros((nq, kstride), dtype=np.float32)
        out_s = np.zeros((nq, kstride), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uintp)
        head = (self._h, _fp(qs), nq, dim, ks_ptr, kscalar, int(candidates), lam_ptr, lscalar)
        tail = (kstride, _u64p(out_ids), _fp(out_d), _fp(out_s), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)))
        if compiled_mask is not None:
            rc = self._L.vdb_flat_search_batch_mmr_filtered(*head, compiled_mask.handle, *tail)
        else:
            mask_ptr = None
            if id_mask is not None:
                m = np.ascontiguousarray(id_mask, dtype=np.uint64)
                mask_ptr = _u64p(m)
            rc = self._L.vdb_flat_search_batch_mmr(*head, mask_ptr, int(mask_bits), *tail)
        if rc:
            _raise(rc)
        return out_ids, out_d, out_s, counts

    def mmr_stats(self):
        """The last search_batch_mmr: [0] queries, [1] the depth the search ran at, [2] candidates summed over the queries,
        [3] pair distances evaluated (sum over the queries of sum_{t=1}^{count-1} (c - t)), [4] rows returned, [5] host ns
        spent turning candidate ids into device rows, [6], [7] 0."""
        out = (ctypes.c_uint64 * 8)()
        rc = self._L.vdb_flat_mmr_stats(self._h, out)
        if rc:
            _raise(rc)
        return [int(x) for x in out]

    # ---- one nearest row per group (include/vdb_flat.h vdb_flat_search_batch_distinct; no reference counterpart)
    def search_batch_distinct(self, queries, k, table, slot, id_mask=None, mask_bits=0, compiled_mask=None):
        """The k nearest GROUPS, each represented by its nearest row: the full ranking of the eligible rows walked from the
        front, a row kept iff its code in column `slot` of `table` (a MetaTable) is -1 or no earlier row has the same code.
        Rows with code -1 (no such field) are never collapsed.  Exact, however deep one group reaches.  k an int or a
        per-query array.  Returns (ids, dists, codes, counts); codes is the int32 group code of every returned row."""
        if compiled_mask is not None and id_mask is not None:
            raise ValueError("pass id_mask or compiled_mask, not both")
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim != 2:
            raise ValueError("queries must be a 2-d array")
        nq, dim = q.shape
        if np.isscalar(k):
            ks_ptr, kscalar, kmax = None, int(k), int(k)
        else:
            ks = np.ascontiguousarray(k, dtype=np.uintp)
            if ks.shape != (nq,):
                raise ValueError(f"k must be a scalar or hold one value per query ({nq}), not {ks.shape}")
            ks_ptr = ks.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
            kscalar, kmax = 0, int(ks.max()) if ks.size else 0
        kstride = max(kmax, 1)
        out_ids = np.zeros((nq, kstride), dtype=np.uint64)
        out_d = np.zeros((nq, kstride), dtype=np.float32)
        out_c = np.full((nq, kstride), -1, dtype=np.int32)
        counts = np.zeros(nq, dtype=np.uintp)
        cp = counts.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
        ccp = out_c.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        t = table._t if table is not None else None
        if compiled_mask is not None:
            rc = self._L.vdb_flat_search_batch_distinct_filtered(self._h, _fp(q), nq, dim, ks_ptr, kscalar, t, int(slot), compiled_mask.handle,
                                                                 kstride, _u64p(out_ids), _fp(out_d), ccp, cp)
        else:
            mask_ptr = None
            if id_mask is not None:
                m = np.ascontiguousarray(id_mask, dtype=np.uint64)
                mask_ptr = _u64p(m)
            rc = self._L.vdb_flat_search_batch_distinct(self._h, _fp(q), nq, dim, ks_ptr, kscalar, t, int(slot), mask_ptr, int(mask_bits),
                                                        kstride, _u64p(out_ids), _fp(out_d), ccp, cp)
        if rc:
            _raise(rc)
        return out_ids, out_d, out_c, counts

    def distinct_stats(self):
        """The last search_batch_distinct: [0] queries, [1] completed by stage A, [2] by stage B, [3] by exclusion rounds,
        [4] exclusion searches run, [5] depth of stage A, [6] depth of stage B, [7] rows returned in total."""
        out = (ctypes.c_uint64 * 8)()
        rc = self._L.vdb_flat_distinct_stats(self._h, out)
        if rc:
            _raise(rc)
        return [int(x) for x in out]

    @staticmethod
    def distinct_depth(k, length, stage):
        """Rows per query the stage-A (0) / stage-B (1) search of search_batch_distinct asks for; needs no device."""
        return int(_ffi.lib().vdb_flat_distinct_depth(int(k), int(length), int(stage)))

    # ---- up to g rows of each of the k nearest groups (include/vdb_flat.h vdb_flat_search_batch_per_group; no reference counterpart)
    PER_GROUP_MAX_SIZE = 32

    def search_batch_per_group(self, queries, k, group_size, table, slot, id_mask=None, mask_bits=0, compiled_mask=None):
        """The k nearest GROUPS (search_batch_distinct's answer under the same arguments) with up to group_size rows of each:
        the members of a group with code c >= 0 are the first group_size rows of the full ranking of the eligible rows whose
        code in column `slot` of `table` is c; a row with code -1 is its own group of one.  Member 0 of every group is its
        representative.  Exact.  k an int or a per-query array.  Returns (ids [nq, k, g], dists [nq, k, g], codes [nq, k],
        sizes [nq, k], counts [nq]); only the first sizes[b, j] members of the first counts[b] groups are meaningful."""
        if compiled_mask is not None and id_mask is not None:
            raise ValueError("pass id_mask or compiled_mask, not both")
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim != 2:
            raise ValueError("queries must be a 2-d array")
        nq, dim = q.shape
        if np.isscalar(k):
            ks_ptr, kscalar, kmax = None, int(k), int(k)
        else:
            ks = np.ascontiguousarray(k, dtype=np.uintp)
            if ks.shape != (nq,):
                raise ValueError(f"k must be a scalar or hold one value per query ({nq}), not {ks.shape}")
            ks_ptr = ks.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
            kscalar, kmax = 0, int(ks.max()) if ks.size else 0
        g = int(group_size)
        kstride, gdim = max(kmax, 1), max(g, 1)
        out_ids = np.zeros((nq, kstride, gdim), dtype=np.uint64)
        out_d = np.zeros((nq, kstride, gdim), dtype=np.float32)
        out_c = np.full((nq, kstride), -1, dtype=np.int32)
        sizes = np.zeros((nq, kstride), dtype=np.uint32)
        counts = np.zeros(nq, dtype=np.uintp)
        tail = (kstride, _u64p(out_ids), _fp(out_d), out_c.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)))
        head = (self._h, _fp(q), nq, dim, ks_ptr, kscalar, g, table._t if table is not None else None, int(slot))
        if compiled_mask is not None:
            rc = self._L.vdb_flat_search_batch_per_group_filtered(*head, compiled_mask.handle, *tail)
        else:
            mask_ptr = None
            if id_mask is not None:
                m = np.ascontiguousarray(id_mask, dtype=np.uint64)
                mask_ptr = _u64p(m)
            rc = self._L.vdb_flat_search_batch_per_group(*head, mask_ptr, int(mask_bits), *tail)
        if rc:
            _raise(rc)
        return out_ids, out_d, out_c, sizes, counts

    def per_group_stats(self):
        """The last search_batch_per_group: [0] queries, [1] groups returned, [2] pairs filled by the member scan, [3] pairs answered
        by a giant's masked search, [4] distinct wanted codes, [5] member rows listed, [6] pair distances evaluated by the fill,
        [7] representative mismatches (always 0)."""
        out = (ctypes.c_uint64 * 8)()
        rc = self._L.vdb_flat_per_group_stats(self._h, out)
        if rc:
            _raise(rc)
        return [int(x) for x in out]

    @staticmethod
    def debug_per_group_plan(codes, kept, ks=None):
        """The host plan of search_batch_per_group for the answers' codes [nq, kmax] and kept counts [nq] (ks: a per-query k);
        needs no device.  Returns (wanted i32 [U] ascending, index u32 [nq, kmax]: the place of every counted entry's code in
        wanted, 0xffffffff for the others), or None for kmax above 1024."""
        cd = np.ascontiguousarray(codes, dtype=np.int32)
        kp = np.ascontiguousarray(kept, dtype=np.uint32).reshape(-1)
        if cd.ndim != 2 or cd.shape[0] != kp.size:
            raise ValueError("codes must be [nq, kmax] and kept [nq]")
        nq, kmax = cd.shape
        i32p, u32p, szp = (ctypes.POINTER(t) for t in (ctypes.c_int32, ctypes.c_uint32, ctypes.c_size_t))
        ksp = None
        if ks is not None:
            ks = np.ascontiguousarray(ks, dtype=np.uintp)
            ksp = ks.ctypes.data_as(szp)
        L = _ffi.lib()
        args = (cd.ctypes.data_as(i32p), kp.ctypes.data_as(u32p), ksp, nq, kmax)
        n = L.vdb_flat_debug_per_group_plan(*args, None, 0, None)
        if n == ctypes.c_size_t(-1).value:
            return None
        wanted = np.zeros(n, dtype=np.int32)
        index = np.zeros((nq, kmax), dtype=np.uint32)
        L.vdb_flat_debug_per_group_plan(*args, wanted.ctypes.data_as(i32p), n, index.ctypes.data_as(u32p))
        return wanted, index

    def debug_set_per_group_scan_cap(self, rows):
        """tests: the longest member list search_batch_per_group's fill takes, in rows (0 = the default, 131072)"""
        rc = self._L.vdb_flat_debug_set_per_group_scan_cap(self._h, int(rows))
        if rc:
            _raise(rc)

    # ---- one batch, a filter per query (include/vdb_flat.h vdb_flat_search_batch_grouped; no reference counterpart)
    def search_batch_grouped(self, queries, k, group_of, id_masks=None, mask_bits=0, compiled_masks=None, ks=None):
        """One batch, a filter per query: the answer for query b is what search_batch_arrays returns for that query alone under
        mask group_of[b] (GROUP_NONE: under no mask) -- ids, order, distance bits and count.  group_of: one mask index per query.
        id_masks: u64 array [n_masks, (mask_bits + 63) // 64]; or compiled_masks: a sequence of CompiledMask (entries no query
        references may be None).  ks: a per-query k (k is then ignored).  The queries that share a mask are answered together, all
        groups in one launch chain.  Returns the arrays of search_batch_arrays."""
        if compiled_masks is not None and id_masks is not None:
            raise ValueError("pass id_masks or compiled_masks, not both")
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim != 2:
            raise ValueError("queries must be a 2-d array")
        nq, dim = q.shape
        if ks is None:
            ks_ptr, kscalar, kmax = None, int(k), int(k)
        else:
            ks = np.ascontiguousarray(ks, dtype=np.uintp)
            if ks.shape != (nq,):
                raise ValueError(f"ks must hold one value per query ({nq}), not {ks.shape}")
            ks_ptr = ks.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
            kscalar, kmax = 0, int(ks.max()) if ks.size else 0
        gp = None
        if group_of is not None:
            go = np.ascontiguousarray(group_of, dtype=np.uint32).reshape(-1)
            if go.shape != (nq,):
                raise ValueError(f"group_of must hold one value per query ({nq}), not {go.shape}")
            gp = go.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        kstride = max(kmax, 1)
        out_ids = np.zeros((nq, kstride), dtype=np.uint64)
        out_d = np.zeros((nq, kstride), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uintp)
        cp = counts.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
        if compiled_masks is not None:
            n_masks = len(compiled_masks)
            arr = (ctypes.c_void_p * max(n_masks, 1))(*[m.handle if m is not None else None for m in compiled_masks])
            rc = self._L.vdb_flat_search_batch_grouped_filtered(self._h, _fp(q), nq, dim, ks_ptr, kscalar, arr if n_masks else None, n_masks,
                                                                gp, kstride, _u64p(out_ids), _fp(out_d), cp)
        else:
            mask_ptr, n_masks = None, 0
            if id_masks is not None:
                m = np.ascontiguousarray(id_masks, dtype=np.uint64)
                words = (int(mask_bits) + 63) // 64
                if m.ndim != 2 or m.shape[1] != words:
                    raise ValueError(f"id_masks must be [n_masks, {words}] for {mask_bits} bits, not {m.shape}")
                n_masks = m.shape[0]
                mask_ptr = _u64p(m) if m.size else None
            rc = self._L.vdb_flat_search_batch_grouped(self._h, _fp(q), nq, dim, ks_ptr, kscalar, mask_ptr, n_masks, int(mask_bits), gp,
                                                       kstride, _u64p(out_ids), _fp(out_d), cp)
        if rc:
            _raise(rc)
        return out_ids, out_d, counts

    def grouped_stats(self):
        """The last search_batch_grouped: [0] queries, [1] masks referenced, [2] queries answered by the grouped scan, [3] by a
        per-group ordinary search, [4] unfiltered queries, [5] eligible rows summed over the scanned groups, [6] tiles launched,
        [7] passes."""
        out = (ctypes.c_uint64 * 8)()
        rc = self._L.vdb_flat_grouped_stats(self._h, out)
        if rc:
            _raise(rc)
        return [int(x) for x in out]

    @staticmethod
    def debug_group_plan(group_of, elig):
        """The plan of a grouped search for these group indices and eligible-row counts (k <= 2048); needs no device.
        Returns (perm u32 [nq], tiles u32 [n_tiles, 4] = group, first list position, first permuted query, queries), or None
        for a group index that is neither below len(elig) nor GROUP_NONE."""
        go = np.ascontiguousarray(group_of, dtype=np.uint32).reshape(-1)
        el = np.ascontiguousarray(elig, dtype=np.uint32).reshape(-1)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        L = _ffi.lib()
        gp, ep = go.ctypes.data_as(u32p) if go.size else None, el.ctypes.data_as(u32p) if el.size else None
        n = L.vdb_flat_debug_group_plan(gp, go.size, ep, el.size, None, None, 0)
        if n == ctypes.c_size_t(-1).value:
            return None
        perm = np.zeros(go.size, dtype=np.uint32)
        tiles = np.zeros((n, 4), dtype=np.uint32)
        L.vdb_flat_debug_group_plan(gp, go.size, ep, el.size, perm.ctypes.data_as(u32p), tiles.ctypes.data_as(u32p), n)
        return perm, tiles

    # ---- bulk build and device-resident entry points
    def add_bulk(self, rows, ids=None, first_id=0):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        n, dim = rows.shape
        idp = None
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.uint64)
            idp = _u64p(ids)
        rc = self._L.vdb_flat_add_bulk(self._h, idp, int(first_id), _fp(rows), n, dim)
        if rc:
            _raise(rc)
        if self._keep:
            for i in range(n):
                self._vectors[int(ids[i]) if ids is not None else first_id + i] = Vector(rows[i])

    def add_bulk_device(self, dev_ptr, n, dim, ids=None, first_id=0):
        """rows already in this GPU's HBM (e.g. a torch tensor's data_ptr()); no host copy is kept."""
        idp = None
        if ids is not None:
            ids = np.ascontiguousarray(ids, dtype=np.uint64)
            idp = _u64p(ids)
        rc = self._L.vdb_flat_add_bulk_device(self._h, idp, int(first_id), ctypes.c_void_p(dev_ptr), int(n), int(dim))
        if rc:
            _raise(rc)

    def load_vector_file(self, path, first_id=0):
        """Bulk-load the reference's mmap vector file (src/persistence/mmap.rs); returns the row count."""
        n = ctypes.c_size_t()
        rc = self._L.vdb_flat_load_vector_file(self._h, os.fsencode(path), int(first_id), ctypes.byref(n))
        if rc:
            _raise(rc)
        return n.value

    def reserve(self, rows, dim):
        rc = self._L.vdb_flat_reserve(self._h, int(rows), int(dim))
        if rc:
            _raise(rc)

    def flush(self):
        rc = self._L.vdb_flat_flush(self._h)
        if rc:
            _raise(rc)

    # ---- reclaiming removed rows (include/vdb_flat.h vdb_flat_compact; no reference counterpart, results identical)
    def compact(self, shrink=False):
        """Move the live device rows down over the removed / overwritten ones, on the device and in place; returns the
        number of device rows given back.  shrink=True also re-allocates the store to a fresh index's capacity.
        A mutation: call it where add / remove are called (the caller's write lock)."""
        got = ctypes.c_size_t(0)
        rc = self._L.vdb_flat_compact(self._h, 1 if shrink else 0, ctypes.byref(got))
        if rc:
            _raise(rc)
        return int(got.value)

    def set_auto_compact(self, fraction):
        """fraction > 0: every flush (so the next search after a write) compacts when more than that share of the uploaded
        rows is dead.  0 (default): never."""
        rc = self._L.vdb_flat_set_auto_compact(self._h, float(fraction))
        if rc:
            _raise(rc)

    def store_stats(self):
        """[0] device rows (live + dead, staged included), [1] live rows, [2] capacity in rows, [3] device bytes of the row
        store, [4] compactions run, [5] rows reclaimed in total, [6] ns of the last compaction (host clock, whole call),
        [7] ns of its device part, [8] chunks it moved directly, [9] chunks it moved through the bounce buffer."""
        out = (ctypes.c_uint64 * 8)()
        rc = self._L.vdb_flat_store_stats(self._h, out)
        if rc:
            _raise(rc)
        v = [int(x) for x in out]
        return v[:7] + [v[7] & ((1 << 40) - 1), v[7] >> 52, (v[7] >> 40) & 4095]

    def debug_set_compact_bounce(self, rows):
        """Test hook: the compaction's bounce buffer in rows (0 = default), so that small indexes exercise many chunks."""
        rc = self._L.vdb_flat_debug_set_compact_bounce(self._h, int(rows))
        if rc:
            _raise(rc)

    @staticmethod
    def debug_compact_plan(live_words, n_rows, bounce_rows=0, ld=32):
        """The chunk plan of a compaction for a live mask (u32 words, bit r & 31 of word r >> 5): an [n, 4] u32 array of
        (first source row, end source row, first destination row, mode 0 direct / 1 bounce).  Needs no device."""
        L = _ffi.lib()
        lw = np.ascontiguousarray(live_words, dtype=np.uint32)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        n = int(L.vdb_flat_debug_compact_plan(lw.ctypes.data_as(u32p), int(n_rows), int(bounce_rows), int(ld), None, 0))
        out = np.zeros((n, 4), dtype=np.uint32)
        if n:
            L.vdb_flat_debug_compact_plan(lw.ctypes.data_as(u32p), int(n_rows), int(bounce_rows), int(ld), out.ctypes.data_as(u32p), n)
        return out

    def search_batch_device(self, q_ptr, nq, dim, k, out_ids_ptr, out_dists_ptr, out_counts_ptr, stream=0,
                            mask_ptr=0, mask_bits=0):
        """Everything resident in HBM: raw device pointers (uint64 ids, f32 dists, u32 counts)."""
        rc = self._L.vdb_flat_search_batch_device(
            self._h, ctypes.c_void_p(q_ptr), int(nq), int(dim), int(k), ctypes.c_void_p(mask_ptr or None),
            int(mask_bits), ctypes.c_void_p(out_ids_ptr), ctypes.c_void_p(out_dists_ptr),
            ctypes.c_void_p(out_counts_ptr), ctypes.c_void_p(stream or None))
        if rc:
            _raise(rc)

    def search_batch_device_begin(self, q_ptr, nq, dim, k, out_ids_ptr, out_dists_ptr, out_counts_ptr, code_ptr=0,
                                  stream=0, mask_ptr=0, mask_bits=0):
        """First tier enqueued, no host synchronisation; *code_ptr (device int32) = 0 or VDB_PENDING_HOST (100).
        Must be followed by search_batch_device_finish() from the same thread."""
        rc = self._L.vdb_flat_search_batch_device_begin(
            self._h, ctypes.c_void_p(q_ptr), int(nq), int(dim), int(k), ctypes.c_void_p(mask_ptr or None),
            int(mask_bits), ctypes.c_void_p(out_ids_ptr), ctypes.c_void_p(out_dists_ptr),
            ctypes.c_void_p(out_counts_ptr), ctypes.c_void_p(code_ptr or None), ctypes.c_void_p(stream or None))
        if rc:
            _raise(rc)

    def search_batch_device_finish(self):
        """Waits, runs the fallback tiers where needed; returns True when outputs were rewritten."""
        changed = ctypes.c_int(0)
        rc = self._L.vdb_flat_search_batch_device_finish(self._h, ctypes.byref(changed))
        if rc:
            _raise(rc)
        return bool(changed.value)

    def search_batch_device_submit(self, q_ptr, nq, dim, k, out_ids_ptr, out_dists_ptr, out_counts_ptr, stream=0,
                                   mask_ptr=0, mask_bits=0):
        """Asynchronous form: the first tier is enqueued, a ticket comes back at once; at most two tickets per handle."""
        t = ctypes.c_int(-1)
        rc = self._L.vdb_flat_search_batch_device_submit(
            self._h, ctypes.c_void_p(q_ptr), int(nq), int(dim), int(k), ctypes.c_void_p(mask_ptr or None),
            int(mask_bits), ctypes.c_void_p(out_ids_ptr), ctypes.c_void_p(out_dists_ptr),
            ctypes.c_void_p(out_counts_ptr), ctypes.c_void_p(stream or None), ctypes.byref(t))
        if rc:
            _raise(rc)
        return t.value

    def search_batch_device_wait(self, ticket):
        """Waits for a submitted search, runs its fallback tiers where needed; its outputs are complete on return."""
        rc = self._L.vdb_flat_search_batch_device_wait(self._h, int(ticket))
        if rc:
            _raise(rc)

    # ---- exact range search (include/vdb_flat.h vdb_flat_range_search_batch; no reference counterpart)
    MAX_RANGE_RESULTS = 2048

    def range_search_batch(self, queries, radius, max_results, id_mask=None, mask_bits=0):
        """Every eligible row whose reference distance d satisfies d <= radius, ascending by (distance, id).
        queries [nq, dim] f32; radius a scalar or a per-query array; max_results in [1, 2048].
        Returns (ids u64 [nq, max_results], dists f32 [nq, max_results], counts [nq], totals u64 [nq]): counts[b] =
        min(totals[b], max_results) entries of row b are written, totals[b] rows lie within the radius."""
        qs = np.ascontiguousarray(queries, dtype=np.float32)
        nq, dim = qs.shape
        mr = int(max_results)
        if np.isscalar(radius):
            rad_ptr, rscalar = None, float(radius)
        else:
            rad = np.ascontiguousarray(radius, dtype=np.float32)
            if rad.shape != (nq,):
                raise ValueError(f"radius must be a scalar or hold one value per query ({nq}), not {rad.shape}")
            rad_ptr, rscalar = _fp(rad), 0.0
        out_ids = np.zeros((nq, max(mr, 1)), dtype=np.uint64)
        out_d = np.zeros((nq, max(mr, 1)), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uintp)
        totals = np.zeros(nq, dtype=np.uint64)
        mask_ptr = None
        if id_mask is not None:
            m = np.ascontiguousarray(id_mask, dtype=np.uint64)
            mask_ptr = _u64p(m)
        rc = self._L.vdb_flat_range_search_batch(self._h, _fp(qs), nq, dim, rad_ptr, ctypes.c_float(rscalar), mask_ptr, int(mask_bits),
                                                 mr, _u64p(out_ids), _fp(out_d),
                                                 counts.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), _u64p(totals))
        if rc:
            _raise(rc)
        return out_ids, out_d, counts, totals

    def range_search_batch_device(self, q_ptr, nq, dim, radii_ptr, max_results, out_ids_ptr, out_dists_ptr, out_counts_ptr,
                                  out_totals_ptr=0, stream=0, mask_ptr=0, mask_bits=0):
        """Everything resident in HBM: raw device pointers (f32 radii [nq], uint64 ids and f32 dists [nq, max_results], u32
        counts, u64 totals or 0).  Unused output slots hold id 2^64 - 1 and a NaN distance."""
        rc = self._L.vdb_flat_range_search_batch_device(
            self._h, ctypes.c_void_p(q_ptr), int(nq), int(dim), ctypes.c_void_p(radii_ptr), ctypes.c_void_p(mask_ptr or None),
            int(mask_bits), int(max_results), ctypes.c_void_p(out_ids_ptr), ctypes.c_void_p(out_dists_ptr),
            ctypes.c_void_p(out_counts_ptr), ctypes.c_void_p(out_totals_ptr or None), ctypes.c_void_p(stream or None))
        if rc:
            _raise(rc)

    def range_stats(self):
        """Counters of the last range search: [0] queries answered by the screened route, [1] by the exact range scan, [2] by
        the dense fallback, [3] rows streamed by filter passes, [4] keys re-ranked, [5] queries whose pool or select
        overflowed, [6] queries without a finite score cut, [7] 0."""
        out = (ctypes.c_uint64 * 8)()
        rc = self._L.vdb_flat_range_stats(self._h, out)
        if rc:
            _raise(rc)
        return [int(x) for x in out]

    def distances_batch(self, queries, id_lists):
        """Exact reference distances of query b to the stored ids id_lists[b] (HNSW candidate lists)."""
        qs = np.ascontiguousarray(queries, dtype=np.float32)
        nq, dim = qs.shape
        offsets = np.zeros(nq + 1, dtype=np.uintp)
        offsets[1:] = np.cumsum([len(l) for l in id_lists])
        ids = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.uint64) for l in id_lists])
                                   if int(offsets[-1]) else np.zeros(0, np.uint64))
        out = np.zeros(int(offsets[-1]), dtype=np.float32)
        rc = self._L.vdb_flat_distances_batch(self._h, _fp(qs), nq, dim,
                                              offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), _u64p(ids), _fp(out))
        if rc:
            _raise(rc)
        return [out[int(offsets[b]):int(offsets[b + 1])] for b in range(nq)]

    def last_stats(self):
        out = (ctypes.c_uint64 * 16)()
        self._L.vdb_flat_last_stats_ex(self._h, out, 16)
        keys = ["mfma_queries", "exact_queries", "pool_overflows", "rows_scanned", "sample_rows", "kprime",
                "uncertified", "fused_kernel_ns", "bf16_screen", "f32_tier_queries", "host_enqueued_ns",
                "host_flags_ns", "host_total_ns", "rethreshold_queries", "shadow_rows", "diag_knobs_active"]
        return dict(zip(keys, [int(v) for v in out]))

    def set_screen(self, mode):
        """1 (default): bf16 screening tier first; 0: f32 MFMA tier only.  Results are identical."""
        rc = self._L.vdb_flat_set_screen(self._h, int(mode))
        if rc:
            _raise(rc)

    def set_split(self, mode=1):
        """The layout of the stored rows: 0 never split, 1 adaptive (default), 2 split before the next eligible screened search.
        Split rows let the screening pass stream 2 bytes per element; every other reader converts them back first.  Results
        are identical in every mode."""
        rc = self._L.vdb_flat_set_split(self._h, int(mode))
        if rc:
            _raise(rc)

    def layout(self):
        """(layout, conversions): 0 = plain f32 rows, 1 = split rows; conversions so far in both directions."""
        out = (ctypes.c_uint64 * 2)()
        rc = self._L.vdb_flat_layout(self._h, out)
        if rc:
            _raise(rc)
        return int(out[0]), int(out[1])

    def debug_set_split_after(self, searches):
        """Test hook: the run of eligible searches after which mode 1 converts (0 = the default)."""
        rc = self._L.vdb_flat_debug_set_split_after(self._h, int(searches))
        if rc:
            _raise(rc)

    def set_wide(self, on=True):
        """Batches above 256 queries: 512 queries per fetch of the rows (default) or 256.  Results are identical."""
        rc = self._L.vdb_flat_set_wide(self._h, 1 if on else 0)
        if rc:
            _raise(rc)

    def set_large_k(self, on=True):
        """112 < k <= 1024 on the screening tier (default) or on the exact scan.  Results are identical."""
        rc = self._L.vdb_flat_set_large_k(self._h, 1 if on else 0)
        if rc:
            _raise(rc)

    # ---- the sparse-filter route of pre-filtered searches (include/vdb_flat.h vdb_flat_set_sparse_filter; results identical)
    SPARSE_NEVER, SPARSE_ALWAYS, SPARSE_AUTO = 0, 1, 2

    def set_sparse_filter(self, mode):
        """Searches with an id mask: 0 (default) the tiers over every row, 1 an exact scan of the eligible rows only whenever
        k <= 2048 and at most 131072 rows are eligible, 2 the same where sparse_limit() says it pays.  Results are identical."""
        mode = int(mode)
        if mode not in (0, 1, 2):
            raise ValueError(f"sparse filter mode must be 0, 1 or 2, not {mode}")
        rc = self._L.vdb_flat_set_sparse_filter(self._h, mode)
        if rc:
            _raise(rc)

    def sparse_stats(self):
        """[0] 1 when the last search was answered by the sparse-filter route, [1] eligible rows of the last masked search made
        with a mode other than 0, [2] searches the route answered since creation, [3] 0."""
        out = (ctypes.c_uint64 * 4)()
        rc = self._L.vdb_flat_sparse_stats(self._h, out)
        if rc:
            _raise(rc)
        return [int(x) for x in out]

    @staticmethod
    def sparse_limit(n_rows, ld, dim, nq):
        """The longest eligible-row list mode 2 sends to the route for that shape (ld: dim rounded up to 32).  Needs no device."""
        return int(_ffi.lib().vdb_flat_sparse_limit(int(n_rows), int(ld), int(dim), int(nq)))

    @staticmethod
    def sparse_tile():
        """(list positions, queries) of one workgroup of the scan kernel."""
        L = _ffi.lib()
        return int(L.vdb_flat_debug_sparse_tile_rows()), int(L.vdb_flat_debug_sparse_tile_queries())

    def debug_eligible_rows(self, mask, mask_bits):
        """Test hook: the ascending device rows a masked search on the route would scan (u32 array); no distance is computed."""
        m = np.ascontiguousarray(mask, dtype=np.uint64)
        if m.size * 64 < int(mask_bits):
            raise ValueError(f"mask holds {m.size * 64} bits, mask_bits is {int(mask_bits)}")
        if m.size == 0:
            m = np.zeros(1, dtype=np.uint64)
        n = ctypes.c_size_t(0)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        rc = self._L.vdb_flat_debug_eligible_rows(self._h, ctypes.c_void_p(m.ctypes.data), int(mask_bits), None, 0, ctypes.byref(n))
        if rc:
            _raise(rc)
        out = np.zeros(int(n.value), dtype=np.uint32)
        if out.size:
            rc = self._L.vdb_flat_debug_eligible_rows(self._h, ctypes.c_void_p(m.ctypes.data), int(mask_bits),
                                                      out.ctypes.data_as(u32p), out.size, ctypes.byref(n))
            if rc:
                _raise(rc)
        return out

    TIERS_NO_RETHRESHOLD, TIERS_FORCE_F32, TIERS_FORCE_EXACT, TIERS_NO_DIRECT = 1, 2, 4, 8
    TIERS_FORCE_RETHRESHOLD = 16

    def set_shadow(self, on=True):
        """Opt-in bf16 shadow of the rows for the screening pass (include/vdb_flat.h: +50 % device memory, half the HBM bytes
        per batch, results identical).  last_stats()["shadow_rows"] tells whether the last search used it."""
        rc = self._L.vdb_flat_set_shadow(self._h, 1 if on else 0)
        if rc != 0:
            _raise(rc)

    def set_sample_cache(self, on=True):
        """The screening tier's compact bf16 copy of its sample rows (include/vdb_flat.h; on by default, results identical)."""
        rc = self._L.vdb_flat_set_sample_cache(self._h, 1 if on else 0)
        if rc != 0:
            _raise(rc)

    def set_tiers(self, flags):
        """Test hook: force the hand-over of queries to the slower tiers (VDB_TIERS_*).  Results are identical."""
        rc = self._L.vdb_flat_set_tiers(self._h, int(flags))
        if rc:
            _raise(rc)

    # ---- certificate diagnostics (include/vdb_flat.h "Diagnostics of the screening tier's CERTIFICATE")
    def debug_screen_scores(self, queries, raw=0, split=False, wide=False):
        """(scores [nq, rows] f32, qinfo [nq, 4], consts dict) from the production filter kernel with open thresholds.
        raw: 0 the scores the screening tier ranks by, 1 its plain scores, 2 the f32 MFMA tier's scores.
        split: over SPLIT rows (an F32 store is converted first and stays SPLIT).  wide: the 512-query kernel (256 < nq <= 512)."""
        qs = np.ascontiguousarray(queries, dtype=np.float32)
        nq, dim = qs.shape
        n = int(self._L.vdb_flat_debug_rows(self._h))
        scores = np.empty((nq, n), dtype=np.float32)
        qinfo = np.zeros((nq, 4), dtype=np.float32)
        consts = np.zeros(8, dtype=np.float64)
        rc = self._L.vdb_flat_debug_screen_scores(self._h, _fp(qs), nq, dim, int(raw) | (4 if split else 0) | (8 if wide else 0), _fp(scores), _fp(qinfo),
                                                  consts.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        if rc:
            _raise(rc)
        keys = ["eps_coef", "c_acc", "kappa", "nd_max", "ed_max", "rho_max", "lower_bound_scores", "ld"]
        return scores, qinfo, dict(zip(keys, consts.tolist()))

    def debug_last_thresholds(self, nq):
        """The screening tier's per-query filter thresholds of the last search (first nq queries)."""
        out = np.zeros(int(nq), dtype=np.float32)
        rc = self._L.vdb_flat_debug_last_thresholds(self._h, _fp(out), int(nq))
        if rc:
            _raise(rc)
        return out

    def debug_row_info(self):
        """[rows, 4] f32: exact-order norm, alpha, beta, margin."""
        n = int(self._L.vdb_flat_debug_rows(self._h))
        out = np.zeros((n, 4), dtype=np.float32)
        rc = self._L.vdb_flat_debug_row_info(self._h, _fp(out), n)
        if rc:
            _raise(rc)
        return out

    def debug_cert_probe(self, qi, T, ek):
        """The production certification test for (prepared query qi[i], score bound T[i], k-th exact distance ek[i])."""
        qi = np.ascontiguousarray(qi, dtype=np.uint32)
        T = np.ascontiguousarray(T, dtype=np.float32)
        ek = np.ascontiguousarray(ek, dtype=np.float32)
        out = np.zeros(qi.size, dtype=np.uint32)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        rc = self._L.vdb_flat_debug_cert_probe(self._h, qi.ctypes.data_as(u32p), _fp(T), _fp(ek), qi.size, out.ctypes.data_as(u32p))
        if rc:
            _raise(rc)
        return out

    def set_profile(self, on=True):
        rc = self._L.vdb_flat_set_profile(self._h, int(bool(on)))
        if rc:
            _raise(rc)

    def dim(self):
        return int(self._L.vdb_flat_dim(self._h))

    # ---- sharded handles (vdb_flat_create_sharded)
    def shards(self):
        return int(self._L.vdb_flat_shards(self._h))

    def shard_len(self, shard):
        return int(self._L.vdb_flat_shard_len(self._h, int(shard)))

    def set_exchange(self, mode):
        """EXCHANGE_RCCL (grouped ncclAllGather over in-process communicators) or EXCHANGE_PEER (peer copies into devices[0])."""
        rc = self._L.vdb_flat_set_exchange(self._h, int(mode))
        if rc:
            _raise(rc)

    def shard_stats(self):
        out = (ctypes.c_uint64 * 8)()
        rc = self._L.vdb_flat_shard_stats(self._h, out)
        if rc:
            _raise(rc)
        keys = ["exchanges", "shards", "exchange_mode", "rccl_ranks", "host_total_ns", "host_enqueued_ns"]
        return dict(zip(keys, [int(v) for v in out]))

"""The sparse-vector index (include/vdb_flat.h "Sparse vectors"): SPLADE / BM25-style weights -- a few dozen
(dimension, weight) pairs out of a large vocabulary -- scored exactly on the device over an inverted file, and the reciprocal-rank
fusion that joins a sparse ranking with a dense one.  There is no CPU search path."""
import ctypes

import numpy as np

from . import _ffi
from .index import _fp, _raise, _u64p

MAX_K, MAX_QUERY_NNZ = 1024, 1024
SEG_ROWS_MAX, SEG_ROWS = 16384, 8192                     # GpuSparseIndex.set_segmented: the largest segment; the default (DESIGN.md 4.20.2 "Measured")
RRF_K = 60


def _csr(vectors):
    """[(indices, values), ...] -> (offsets uintp [n + 1], indices u32, values f32); a pair of unequal lengths is refused"""
    offs = np.zeros(len(vectors) + 1, dtype=np.uintp)
    idx, val = [], []
    for i, (ind, v) in enumerate(vectors):
        ind = np.asarray(ind).reshape(-1)
        v = np.asarray(v, dtype=np.float32).reshape(-1)
        if ind.size != v.size:
            raise ValueError(f"sparse vector {i}: {ind.size} indices but {v.size} values")
        if ind.size and (ind.min() < 0 or ind.max() >= 1 << 32):
            raise ValueError(f"sparse vector {i}: an index does not fit 32 bits")
        idx.append(ind.astype(np.uint32))
        val.append(v)
        offs[i + 1] = offs[i] + ind.size
    cat = (lambda parts, dt: np.ascontiguousarray(np.concatenate(parts), dtype=dt) if parts else np.zeros(0, dtype=dt))
    return offs, cat(idx, np.uint32), cat(val, np.float32)


def rrf_fuse(rankings, k):
    """Reciprocal-rank fusion of ranked id lists (best first): score(id) = the sum over the lists that hold it of
    1 / (60 + rank), rank counted from 1, in f64, summed in the order of the lists; the k best by (score descending, id
    ascending) as [(id, score), ...]."""
    score = {}
    for ids in rankings:
        for r, i in enumerate(ids):
            score[i] = score.get(i, 0.0) + 1.0 / (RRF_K + r + 1)
    return sorted(score.items(), key=lambda kv: (-kv[1], kv[0]))[:int(k)]


class GpuSparseIndex:
    """Sparse vectors by id on one GPU.  score(q, x) = the f32 fold of q_d * x_d over the shared indices in ascending order,
    distance = -score; a stored vector that shares no index with the query is never returned."""

    def __init__(self, device=0):
        self._L = _ffi.lib()
        self._h = ctypes.c_void_p()
        rc = self._L.vdb_spv_create(int(device), ctypes.byref(self._h))
        if rc:
            _raise(rc)
        self._device = int(device)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.vdb_spv_destroy(h)

    __del__ = close

    def add_bulk(self, ids, vectors):
        """ids: u64 array; vectors: one (indices, values) pair per id, in any index order.  An existing id is overwritten."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        if ids.size != len(vectors):
            raise ValueError(f"{ids.size} ids but {len(vectors)} vectors")
        self.add_csr(ids, *_csr(vectors))

    def add_csr(self, ids, offsets, indices, values):
        """add_bulk from CSR arrays: row i owns the pairs [offsets[i], offsets[i + 1]) of indices / values."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        offs = np.ascontiguousarray(offsets, dtype=np.uintp).reshape(-1)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        val = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        if offs.size != ids.size + 1 or idx.size != val.size or (ids.size and int(offs[-1]) > idx.size):
            raise ValueError("offsets, indices and values do not describe one vector per id")
        rc = self._L.vdb_spv_add_bulk(self._h, _u64p(ids), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)),
                                      idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), _fp(val), ids.size)
        if rc:
            _raise(rc)

    def add(self, id, indices, values):
        self.add_bulk([id], [(indices, values)])

    def remove(self, id):
        rc = self._L.vdb_spv_remove(self._h, int(id))
        if rc:
            _raise(rc)

    def len(self):
        return int(self._L.vdb_spv_len(self._h))

    __len__ = len

    def flush(self):
        """Rebuild the inverted file now (the next search does it otherwise)."""
        rc = self._L.vdb_spv_flush(self._h)
        if rc:
            _raise(rc)

    def search_batch_arrays(self, queries, k, id_mask=None, mask_bits=0, compiled_mask=None):
        """queries: [(indices, values), ...]; k an int or a per-query array, at most 1024.  Returns (ids u64 [nq, kmax],
        dists f32 [nq, kmax], counts [nq]); id_mask / mask_bits / compiled_mask as GpuFlatIndex.search_batch_arrays."""
        if compiled_mask is not None and id_mask is not None:
            raise ValueError("pass id_mask or compiled_mask, not both")
        offs, idx, val = _csr(queries)
        nq = len(queries)
        if np.isscalar(k):
            ks_ptr, kscalar, kmax = None, int(k), int(k)
        else:
            ks = np.ascontiguousarray(k, dtype=np.uintp)
            if ks.shape != (nq,):
                raise ValueError("k must be an int or one value per query")
            ks_ptr = ks.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t))
            kscalar, kmax = 0, int(ks.max()) if ks.size else 0
        kstride = max(kmax, 1)
        out_ids = np.zeros((nq, kstride), dtype=np.uint64)
        out_d = np.zeros((nq, kstride), dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uintp)
        head = (self._h, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                _fp(val), nq, ks_ptr, kscalar)
        tail = (kstride, _u64p(out_ids), _fp(out_d), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)))
        if compiled_mask is not None:
            rc = self._L.vdb_spv_search_batch_filtered(*head, compiled_mask.handle, *tail)
        else:
            m = np.ascontiguousarray(id_mask, dtype=np.uint64) if id_mask is not None else None
            rc = self._L.vdb_spv_search_batch(*head, _u64p(m) if m is not None else None, int(mask_bits), *tail)
        if rc:
            _raise(rc)
        return out_ids, out_d, counts

    def search(self, indices, values, k, id_mask=None, mask_bits=0):
        ids, d, c = self.search_batch_arrays([(indices, values)], int(k), id_mask=id_mask, mask_bits=mask_bits)
        return [(int(ids[0, i]), np.float32(d[0, i])) for i in range(int(c[0]))]

    def stats(self):
        out = (ctypes.c_uint64 * 8)()
        rc = self._L.vdb_spv_stats(self._h, out)
        if rc:
            _raise(rc)
        names = ("rows", "dead_rows", "nnz", "vocab", "rebuilds", "entries_walked", "candidates", "chunks")
        return dict(zip(names, (int(x) for x in out)))

    def set_route(self, mode):
        """How searches score: 0 the inverted-file walk (default), 1 the row-major route (batches that hold the frequent words),
        2 whichever has less counted work (route_stats; the factor is route_rho()).  The answers are the same to the bit."""
        rc = self._L.vdb_spv_set_route(self._h, int(mode))
        if rc:
            _raise(rc)

    def route_stats(self):
        """of the last search: the route taken, its row passes, and the counted work of either route"""
        out = (ctypes.c_uint64 * 4)()
        rc = self._L.vdb_spv_route_stats(self._h, out)
        if rc:
            _raise(rc)
        return dict(zip(("route", "passes", "work_inverted", "work_rows"), (int(x) for x in out)))

    def route_rho(self):
        return float(self._L.vdb_spv_route_rho())

    def set_segmented(self, rows=SEG_ROWS):
        """How the inverted route walks: 0 one workgroup per query (default); a power of two in [64, 16384] one workgroup per
        (query, segment of that many rows) with the accumulators in LDS, for requests of a few queries (segment_stats says whether
        it ran: a store needs two segments).  The answers are the same to the bit; a change rebuilds the inverted file."""
        rc = self._L.vdb_spv_set_segmented(self._h, int(rows))
        if rc:
            _raise(rc)

    def segment_stats(self):
        """of the last search: whether the segmented walk ran, its segments, rows per segment, and the (query, segment) workgroups
        that found a posting"""
        out = (ctypes.c_uint64 * 4)()
        rc = self._L.vdb_spv_segment_stats(self._h, out)
        if rc:
            _raise(rc)
        return dict(zip(("segmented", "segments", "rows_per_segment", "workgroups"), (int(x) for x in out)))

    def debug_set_workspace_cap(self, nbytes):
        """Lower the accumulator workspace (tests: several chunks on a small index); 0 restores 256 MiB."""
        rc = self._L.vdb_spv_debug_set_workspace_cap(self._h, int(nbytes))
        if rc:
            _raise(rc)

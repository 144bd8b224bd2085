"""The binary flat index (include/vdb_flat.h "Binary vectors"): rows of packed bits under Hamming or Jaccard
distance, kept packed on the device, widened in registers and counted exactly on its integer matrix cores.  There is no CPU
search path."""
import ctypes
import enum

import numpy as np

from . import _ffi
from .index import _fp, _raise, _u64p

MAX_K, MAX_DIM = 1024, 32768


class BinaryMetric(enum.IntEnum):
    Hamming = 0
    Jaccard = 1


def as_uint8(a, what):
    """a as a C-contiguous np.uint8 array of packed bits; any other dtype is a TypeError, never a cast"""
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise TypeError(f"{what} must be np.uint8 (packed bits), not {a.dtype}: a binary index never casts")
    return np.ascontiguousarray(a)


def _u8p(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


class GpuBinaryIndex:
    """dim-bit vectors by id on one GPU, passed packed as np.uint8 [.., dim / 8].  With a = popcount(q & x), h = popcount(q ^ x)
    and u = popcount(q | x) as exact integers the distance is (f32)h (Hamming) or 1 - (f32)a / (f32)u, 0 where u = 0 (Jaccard);
    ties go to the smaller id."""

    def __init__(self, metric, device=0):
        self._L = _ffi.lib()
        self._h = ctypes.c_void_p()
        rc = self._L.vdb_bin_create(int(metric), int(device), ctypes.byref(self._h))
        if rc:
            _raise(rc)
        self._metric, self._device = BinaryMetric(metric), int(device)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.vdb_bin_destroy(h)

    __del__ = close

    def add_bulk(self, ids, rows):
        """ids: u64 array; rows: np.uint8 [n, dim / 8].  An existing id is overwritten."""
        rows = as_uint8(rows, "rows")
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        if rows.ndim != 2 or rows.shape[0] != ids.size:
            raise ValueError(f"{ids.size} ids but rows of shape {rows.shape}")
        rc = self._L.vdb_bin_add_bulk(self._h, _u64p(ids), _u8p(rows), ids.size, rows.shape[1] * 8)
        if rc:
            _raise(rc)

    def add(self, id, row):
        self.add_bulk([id], as_uint8(row, "row").reshape(1, -1))

    def remove(self, id):
        rc = self._L.vdb_bin_remove(self._h, int(id))
        if rc:
            _raise(rc)

    def len(self):
        return int(self._L.vdb_bin_len(self._h))

    __len__ = len

    def flush(self):
        """Send ids, id ranks and live bits to the device now (the next search does it otherwise)."""
        rc = self._L.vdb_bin_flush(self._h)
        if rc:
            _raise(rc)

    def search_batch_arrays(self, queries, k, id_mask=None, mask_bits=0, compiled_mask=None):
        """queries: np.uint8 [nq, dim / 8]; k an int or a per-query array, at most 1024.  Returns (ids u64 [nq, kmax], dists f32
        [nq, kmax], counts [nq]); id_mask / mask_bits / compiled_mask as GpuFlatIndex.search_batch_arrays."""
        if compiled_mask is not None and id_mask is not None:
            raise ValueError("pass id_mask or compiled_mask, not both")
        queries = as_uint8(queries, "queries")
        if queries.ndim != 2:
            raise ValueError(f"queries of shape {queries.shape}: [nq, dim / 8] expected")
        nq = queries.shape[0]
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
        head = (self._h, _u8p(queries), nq, queries.shape[1] * 8, ks_ptr, kscalar)
        tail = (kstride, _u64p(out_ids), _fp(out_d), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)))
        if compiled_mask is not None:
            rc = self._L.vdb_bin_search_batch_filtered(*head, compiled_mask.handle, *tail)
        else:
            m = np.ascontiguousarray(id_mask, dtype=np.uint64) if id_mask is not None else None
            rc = self._L.vdb_bin_search_batch(*head, _u64p(m) if m is not None else None, int(mask_bits), *tail)
        if rc:
            _raise(rc)
        return out_ids, out_d, counts

    def search(self, query, k, id_mask=None, mask_bits=0):
        ids, d, c = self.search_batch_arrays(as_uint8(query, "query").reshape(1, -1), int(k), id_mask=id_mask, mask_bits=mask_bits)
        return [(int(ids[0, i]), np.float32(d[0, i])) for i in range(int(c[0]))]

    def stats(self):
        """merge_keys depends on the order in which workgroups published their thresholds: it varies from call to call"""
        out = (ctypes.c_uint64 * 8)()
        rc = self._L.vdb_bin_stats(self._h, out)
        if rc:
            _raise(rc)
        names = ("rows", "dead_rows", "dim", "ld", "segments", "workgroups", "merge_keys")
        st = dict(zip(names, (int(x) for x in out)))
        st["rows_per_segment"], st["query_tile"] = int(out[7]) & 0xffffffff, int(out[7]) >> 32
        return st

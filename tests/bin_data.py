"""The binary index's definition (include/vdb_flat.h "Binary vectors") in numpy: popcounts by a 256-entry table, the distance
through np.float32 operations in the stated order, the answer by np.lexsort over (distance bits, id as uint64)."""
import numpy as np

F32, U64, U8 = np.float32, np.uint64, np.uint8
HAMMING, JACCARD = 0, 1
POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def distances(metric, q, rows):
    """f32 [n]: the distances of the packed rows [n, dim / 8] from the packed query [dim / 8]"""
    a, h = POP[rows & q].sum(axis=1), POP[rows ^ q].sum(axis=1)
    if metric == HAMMING:
        return h.astype(F32)
    u = h + a                                            # popcount(q | x)
    return np.where(u == 0, F32(0.0), F32(1.0) - a.astype(F32) / np.maximum(u, 1).astype(F32)).astype(F32)


def search(metric, ids, rows, live, queries, ks, eligible=None):
    """[(ids u64, dists f32), ...] per query over the live (and eligible) rows; ks an int or one k per query"""
    ids, live = np.asarray(ids, dtype=U64), np.asarray(live, dtype=bool)
    ks = np.full(len(queries), ks) if np.isscalar(ks) else np.asarray(ks)
    keep = np.flatnonzero(live if eligible is None else live & eligible)
    out = []
    for q, k in zip(queries, ks):
        d = distances(metric, q, rows[keep])
        order = np.lexsort((ids[keep], d.view(np.uint32)))[:int(k)]      # d >= +0: the bits order as the distances do
        out.append((ids[keep][order], d[order]))
    return out


def check(ix, metric, ids, rows, live, queries, ks, mask=None, **how):
    """ix.search_batch_arrays against search(): ids, order, distance bits and counts.  mask: the eligible rows (bool per row);
    how: the id_mask / mask_bits / compiled_mask that says so to the index"""
    want = search(metric, ids, rows, live, queries, ks, mask)
    got_ids, got_d, counts = ix.search_batch_arrays(queries, ks, **how)
    for b, (wi, wd) in enumerate(want):
        assert counts[b] == wi.size, (b, counts[b], wi.size)
        assert np.array_equal(got_ids[b, :wi.size], wi), (b, got_ids[b, :wi.size][:8], wi[:8])
        assert np.array_equal(got_d[b, :wi.size].view(np.uint32), wd.view(np.uint32)), (b, got_d[b, :wi.size][:8], wd[:8])
    return got_ids, got_d, counts


def random_rows(rng, n, dim, density):
    """packed rows [n, dim / 8] whose bits are set with probability density"""
    return np.packbits(rng.random((n, dim)) < density, axis=1)

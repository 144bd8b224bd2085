"""The sparse-vector search restated in numpy (include/vdb_flat.h "Sparse vectors"), and a seeded builder of small corpora.

Rows are held densified -- X[row, d] the value, P[row, d] whether the row has index d (an explicit zero has) -- so one query is
a loop over its indices in ascending order with one f32 multiply and one f32 add per step, over all rows at once."""
import numpy as np

VOCAB = 512


class NanScore(Exception):
    pass


def ordered(d):
    """the index's order-preserving map f32 -> u32 (-0.0 in front of +0.0)"""
    b = np.asarray(d, dtype=np.float32).view(np.uint32)
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def scores(X, P, query):
    """(touched bool [n], s f32 [n]): s = 0.0f; for d in the shared indices, ascending: s = s + (q_d * x_d)"""
    idx, val = np.asarray(query[0], dtype=np.int64), np.asarray(query[1], dtype=np.float32)
    s = np.zeros(X.shape[0], dtype=np.float32)
    touched = np.zeros(X.shape[0], dtype=bool)
    with np.errstate(all="ignore"):
        for j in np.argsort(idx, kind="stable"):
            if idx[j] < X.shape[1]:
                m = P[:, idx[j]]
                s[m] = s[m] + val[j] * X[m, idx[j]]
                touched |= m
    return touched, s


def search(ids, X, P, query, k, eligible=None):
    """the k candidates by (distance = -s, id): (ids u64, dists f32); NanScore if an eligible candidate's score is NaN"""
    touched, s = scores(X, P, query)
    if eligible is not None:
        touched &= eligible
    rows = np.flatnonzero(touched)
    if np.isnan(s[rows]).any():
        raise NanScore()
    d = -s[rows]
    order = np.lexsort((ids[rows], ordered(d)))[:k]
    return ids[rows][order], d[order]


def vectors(X, P):
    """the rows as (indices, values) pairs, indices in DESCENDING order (the index sorts on entry)"""
    return [(np.flatnonzero(p)[::-1].astype(np.uint32), x[np.flatnonzero(p)[::-1]]) for x, p in zip(X, P)]


def id_mask(ids, eligible, bits):
    """the id bitmask (u64 words, LSB first) that admits exactly the eligible rows with an id below `bits`"""
    m = np.zeros((bits + 63) // 64, dtype=np.uint64)
    for i in ids[eligible & (ids < bits)]:
        m[int(i) >> 6] |= np.uint64(1) << np.uint64(int(i) & 63)
    return m


def corpus(seed=0, n=6000):
    """ids u64 [n] (shuffled, some >= 2^32), X f32 [n, VOCAB], P bool: 1-40 indices per row out of 0..479 without 100; indices
    7, 8 and 9 each in about 2500 rows; rows 10-13 identical (ids on both sides of 2^32); negative weights; row 20 has an
    explicit zero at index 7; rows 30-39 hold only index 470, which no other row has."""
    rng = np.random.default_rng(seed)
    X = np.zeros((n, VOCAB), dtype=np.float32)
    P = np.zeros((n, VOCAB), dtype=bool)
    pool = np.array([d for d in range(480) if d not in (7, 8, 9, 100, 470)])
    for r in range(n):
        P[r, rng.choice(pool, size=rng.integers(1, 38), replace=False)] = True
    for d in (7, 8, 9):
        P[rng.choice(n, size=2500 + 20 * d, replace=False), d] = True
    P[30:40] = False
    P[30:40, 470] = True
    X[P] = rng.standard_normal(int(P.sum())).astype(np.float32)
    X[10] *= 16                                          # (so that a query equal to row 10 ranks the four copies first)
    P[11:14] = P[10]
    X[11:14] = X[10]
    P[20, 7], X[20, 7] = True, 0.0
    ids = (rng.permutation(n).astype(np.uint64) * np.uint64(3) + np.uint64(1))
    ids[11], ids[12], ids[13] = (1 << 32) + 5, (1 << 63) + 1, 2      # ids[10] stays small: the tie order crosses 2^32
    return ids, X, P


# ------------------------------------------------------------------ the same definition over CSR rows (no dense block)
def csc_view(offsets, indices):
    """(order, sorted indices, row of every entry): the entries grouped by index, rows ascending inside one index"""
    offsets = np.asarray(offsets, dtype=np.int64)
    indices = np.asarray(indices)
    row_of = np.repeat(np.arange(offsets.size - 1, dtype=np.int64), np.diff(offsets))
    order = np.argsort(indices, kind="stable")
    return order, indices[order], row_of


def fold_csr(offsets, indices, values, live, query, view=None):
    """(touched bool [n], s f32 [n], entries walked): the fold of `scores` over the live rows of a CSR log; a dead row is in no
    list.  One pass per query index, ascending; no loop over rows."""
    order, sidx, row_of = view if view is not None else csc_view(offsets, indices)
    values = np.asarray(values, dtype=np.float32)
    live = np.asarray(live, dtype=bool)
    idx, val = np.asarray(query[0], dtype=np.int64), np.asarray(query[1], dtype=np.float32)
    s = np.zeros(live.size, dtype=np.float32)
    touched = np.zeros(live.size, dtype=bool)
    walked = 0
    with np.errstate(all="ignore"):
        for j in np.argsort(idx, kind="stable"):
            e = order[np.searchsorted(sidx, idx[j], "left"):np.searchsorted(sidx, idx[j], "right")]
            e = e[live[row_of[e]]]
            rows = row_of[e]
            s[rows] = s[rows] + val[j] * values[e]
            touched[rows] = True
            walked += rows.size
    return touched, s, walked


def search_csr(ids, offsets, indices, values, live, query, k, eligible=None, view=None, counters=None):
    """`search` over a CSR log with a live flag per row: the same candidate rule, NaN rule and (ordered(-s), id) order.
    counters (a dict), when given, receives entries_walked and candidates, also when NanScore is raised."""
    ids = np.asarray(ids, dtype=np.uint64)
    touched, s, walked = fold_csr(offsets, indices, values, live, query, view)
    if eligible is not None:
        touched &= eligible
    rows = np.flatnonzero(touched)
    if counters is not None:
        counters["entries_walked"] = counters.get("entries_walked", 0) + walked
        counters["candidates"] = counters.get("candidates", 0) + rows.size
    if np.isnan(s[rows]).any():
        raise NanScore()
    d = -s[rows]
    order = np.lexsort((ids[rows], ordered(d)))[:k]
    return ids[rows][order], d[order]


def csr_of(vectors):
    """[(indices, values), ...] -> (offsets i64 [n + 1], indices u32, values f32), the pairs in the order given"""
    offs = np.zeros(len(vectors) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(v[0]) for v in vectors])
    cat = (lambda parts, dt: np.concatenate([np.asarray(p, dtype=dt).reshape(-1) for p in parts]) if parts else np.zeros(0, dtype=dt))
    return offs, cat([v[0] for v in vectors], np.uint32), cat([v[1] for v in vectors], np.float32)


def dense_of(offsets, indices, values, vocab):
    """the CSR rows densified for `search`: (X f32 [n, vocab], P bool)"""
    n = len(offsets) - 1
    X, P = np.zeros((n, vocab), dtype=np.float32), np.zeros((n, vocab), dtype=bool)
    row_of = np.repeat(np.arange(n), np.diff(offsets))
    X[row_of, indices], P[row_of, indices] = values, True
    return X, P


def csr_from_dense(X, P):
    """(offsets, indices, values) of a dense block, indices DESCENDING inside a row as `vectors` gives them"""
    return csr_of(vectors(X, P))


def big_mask(ids, eligible, bits):
    """id_mask without a Python loop (ids below `bits` only)"""
    on = np.zeros(((bits + 63) // 64) * 64, dtype=np.uint8)
    on[np.asarray(ids)[eligible & (ids < bits)].astype(np.int64)] = 1
    return np.packbits(on, bitorder="little").view(np.uint64)


def check_csr(ix, C, queries, k, eligible=None, mask=None, bits=0, view=None, compiled=None):
    """one batch on a GpuSparseIndex against search_csr: counts, ids, order, distance bits, entries_walked and candidates.
    C = (ids, offsets, indices, values, live)."""
    ids, offsets, indices, values, live = C
    view = view if view is not None else csc_view(offsets, indices)
    out_ids, out_d, counts = ix.search_batch_arrays(queries, k, id_mask=mask, mask_bits=bits, compiled_mask=compiled)
    ks = np.full(len(queries), k) if np.isscalar(k) else k
    ctr = {}
    for b, q in enumerate(queries):
        ei, ed = search_csr(ids, offsets, indices, values, live, q, int(ks[b]), eligible, view, ctr)
        assert counts[b] == ei.size, (b, counts[b], ei.size)
        assert np.array_equal(out_ids[b, :ei.size], ei), b
        assert np.array_equal(out_d[b, :ei.size].view(np.uint32), ed.view(np.uint32)), b
    st = ix.stats()
    if len(queries) and int(np.max(ks)) > 0 and live.any() and sum(len(q[0]) for q in queries):
        assert (st["entries_walked"], st["candidates"]) == (ctr["entries_walked"], ctr["candidates"]), (st, ctr)
    return out_ids, out_d, counts


# ------------------------------------------------------------------ weights at the edges of f32
DEN, TINY, FMAX, INF = np.float32(2.0 ** -149), np.float32(2.0 ** -126), np.finfo(np.float32).max, np.float32(np.inf)
NAN_PAYLOADS = (0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffbeef, 0xffffbeef)     # 0x7fffbeef: the accumulators' "untouched" pattern


def _nan(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


_EDGE = None


def edge_corpus():
    """A hand-built corpus of weights at the edges of f32, vocabulary 96, as a dict:
      ids, offsets, indices, values   the rows (CSR, indices NOT sorted inside a row), ids shuffled with some >= 2^32
      row                              name -> row number
      finite                           [(name, query, {row name: expected score bits})]: queries no row turns into NaN
      nan                              [(name, query, [names of the rows whose score is NaN])]
    Dimensions 0-3 serve the finite queries "fold" = {0: 2^-20, 1: 1, 2: 1, 3: 1} (given unsorted) and "den_query" =
    {1: 2^-149}; dimension 5 serves "inf_query" = {5: +inf}; 40 gaussian rows over dimensions 0-3 and 6-9 stand among them.
    Every NaN case owns dimensions of its own from 16 on, so that no finite query meets a NaN."""
    global _EDGE
    if _EDGE is not None:
        return _EDGE
    f = np.float32
    rows, finite, nan = [], [], []

    def row(name, pairs):
        rows.append((name, [d for d, _ in pairs], [v for _, v in pairs]))

    p60 = f(2.0 ** 60)
    row("den_product", [(0, f(2.0 ** -120))])                           # 2^-140
    row("underflow_pos", [(0, f(2.0 ** -140))])                         # 2^-160 -> +0
    row("underflow_neg", [(0, f(-2.0 ** -140))])                        # -> -0; 0.0 + -0.0 = +0.0
    row("den_mid", [(2, TINY), (0, f(2.0 ** -120)), (1, f(2.0 ** -130))])   # 2^-140, + 2^-130 (denormal), + 2^-126: normal
    row("overflow_pos", [(2, FMAX), (1, FMAX)])
    row("overflow_neg", [(1, -FMAX), (2, -FMAX)])
    row("inf_stays", [(3, -FMAX), (1, FMAX), (2, FMAX)])                # inf + -FLT_MAX = inf
    row("cancel_a", [(3, -p60), (1, p60), (2, f(1.0))])                 # (2^60 + 1) - 2^60 = 0
    row("cancel_b", [(3, f(1.0)), (2, -p60), (1, p60)])                 # (2^60 - 2^60) + 1 = 1
    row("cancel_c", [(2, p60), (3, -p60), (1, f(1.0))])                 # (1 + 2^60) - 2^60 = 0
    row("stored_inf", [(1, INF)])
    row("stored_ninf", [(1, -INF)])
    row("smallest_normal", [(1, TINY)])
    row("largest_normal", [(1, FMAX)])
    row("smallest_denormal", [(1, DEN)])
    row("minus_zero", [(1, f(-0.0))])
    row("plus_zero", [(1, f(0.0))])
    row("den_query_big", [(1, f(2.0 ** 20))])                           # * 2^-149 = 2^-129: a denormal product from the query side
    row("inf_query_pos", [(5, f(2.0))])
    row("inf_query_neg", [(5, f(-1.0))])
    rng = np.random.default_rng(420)
    pool = np.array([0, 1, 2, 3, 6, 7, 8, 9])
    for i in range(40):
        d = rng.permutation(pool)[:rng.integers(1, 6)]
        row("tame%d" % i, list(zip(d.tolist(), rng.standard_normal(d.size).astype(f))))
    bits = (lambda x: int(np.array([x], dtype=f).view(np.uint32)[0]))
    finite.append(("fold", (np.array([2, 0, 3, 1], np.uint32), np.array([1.0, 2.0 ** -20, 1.0, 1.0], f)), {
        "den_product": bits(2.0 ** -140), "underflow_pos": 0, "underflow_neg": 0,
        "den_mid": bits(2.0 ** -126 + 2.0 ** -130 + 2.0 ** -140), "overflow_pos": 0x7f800000, "overflow_neg": 0xff800000,
        "inf_stays": 0x7f800000, "cancel_a": 0, "cancel_b": bits(1.0), "cancel_c": 0, "stored_inf": 0x7f800000,
        "stored_ninf": 0xff800000, "smallest_normal": bits(TINY), "largest_normal": bits(FMAX), "smallest_denormal": 1,
        "minus_zero": 0, "plus_zero": 0}))
    finite.append(("den_query", (np.array([1], np.uint32), np.array([DEN], f)), {
        "den_query_big": bits(2.0 ** -129), "largest_normal": bits(2.0 ** -21 - 2.0 ** -45), "smallest_normal": 0, "minus_zero": 0}))      # 0.0 + -0.0 = +0.0
    finite.append(("neg_query", (np.array([1], np.uint32), np.array([-1.0], f)), {
        "plus_zero": 0, "minus_zero": 0, "stored_inf": 0xff800000, "smallest_denormal": 0x80000001}))
    finite.append(("inf_query", (np.array([5], np.uint32), np.array([INF], f)), {"inf_query_pos": 0x7f800000, "inf_query_neg": 0xff800000}))
    dim = [16]

    def case(name, stored, query, bystander=None):
        d0 = dim[0]
        dim[0] += 4
        row(name, [(d0 + j, v) for j, v in reversed(list(enumerate(stored)))])
        if bystander is not None:
            row(name + "_by", [(d0, f(bystander))])
        nan.append((name, (np.array([d0 + j for j in range(len(query))][::-1], np.uint32), np.array(query[::-1], f)), [name]))

    case("zero_times_stored_inf", [INF], [0.0], 2.0)
    case("query_inf_times_zero", [f(0.0)], [INF], 2.0)
    case("inf_minus_inf", [INF, -INF], [1.0, 1.0], 3.0)
    case("inf_minus_inf_by_sign", [INF, INF], [1.0, -1.0], 3.0)
    case("nan_then_finite", [_nan(0x7fffbeef), f(1.0)], [1.0, 1.0], 1.0)
    for pl in NAN_PAYLOADS:
        case("stored_nan_%08x" % pl, [_nan(pl)], [1.0], 1.0)
        case("query_nan_%08x" % pl, [f(1.0)], [_nan(pl)])
    offsets, indices, values = csr_of([(r[1], r[2]) for r in rows])
    n = len(rows)
    ids = rng.permutation(n).astype(np.uint64) * np.uint64(7) + np.uint64(3)
    ids[[1, 5, n - 2]] += np.uint64(1 << 32)
    ids[7] += np.uint64(1 << 63)
    for a in (ids, offsets, indices, values):
        a.setflags(write=False)
    _EDGE = {"ids": ids, "offsets": offsets, "indices": indices, "values": values, "row": {r[0]: i for i, r in enumerate(rows)},
             "finite": finite, "nan": nan, "vocab": 96}
    return _EDGE

"""Value families for the tests at the edges of f32 (tests/test_value_edges_cpu.py, tests/test_gpu_value_edges.py).

Each family is a function (rng, n, d, nq, metric) -> rows f32[n, d], queries f32[nq, d]; ids are the row numbers.  What the
ORACLE's answer contains for each is stated here and pinned, shape by shape, by tests/test_value_edges_cpu.py; the GPU tests
then only have to equal the oracle bit for bit.  Every family leaves rows 0 .. 7 inside its widest tie group and keeps
HIDDEN(n) = n // 3 for the one row an error family hides, so that one set of tombstones (dead_rows) and one set of rows a
mask always excludes (masked_out) serve all of them: the lowest ids of a tie group are never simply 0, 1, 2, ...

  inf_tail  (Euclid, Dot)   all rows but F_FINITE = 5 carry one +inf element; the query is positive there.  Euclid: the live
            finite rows first, then +inf ordered by id.  Dot: the whole top-k is -inf, ordered by id.
  overflow  (all metrics)   finite elements; about 1 % of the rows (at least 160) overflow: half carry ~3e19 (a square is inf),
            half ~2e38 (a sum of two is inf).  Query 0 overflows its own norm.  Euclid: +inf for such a row (never inside a
            tame query's top-k) and for EVERY row under query 0: one tie group, ids decide.  Dot (all signs equal where it
            counts): -inf first, ids decide.  Cosine: the row norm is inf and the dot finite, sim = 0, the distance exactly
            1.0; the tame rows point away from the queries (distance > 1), so the top-k is the 1.0 group, ids decide.
  subnormal (Euclid, Dot)   Euclid: half the rows are small integers times 1e-23, half gaussian (times 3).  Even queries are tiny too:
            sums of squares are 0 or subnormal (the square root of a subnormal is a small normal number), many exact 0.0.
            Odd queries are gaussian: q - x == q for every tiny row, one tie group of n / 2 rows at the normal distance
            |q| whose x*x terms are subnormal.  Dot: every row is small integers times 1e-22; even queries likewise:
            products are multiples of 2^-149, distances subnormal or -0.0; odd queries gaussian.
  cos_den_tiny (Cosine)     half the rows are small integers times 5e-23 (norms at the bottom of f32: a norm of 1e-25 cannot
            exist, the smallest positive sum of squares is 2^-149 and its root 3.7e-23) along the even queries, which are integers
            times 1e-20: n1 * n2 is SUBNORMAL and so is the dot; 0 / 0 cannot arise with both norms positive (2^-74.5 squared rounds to 2^-149, not
            to 0), the quotient is coarse and often leaves [-1, 1].  No error.
  cos_den_zero (Cosine)     row HIDDEN is 1e-25 in every element: not a zero row, but its norm underflows to 0.  The oracle
            answers InvalidVector while the row is alive and eligible, and succeeds once it is hidden.
  (no cos_den_inf)          n1 * n2 = inf between FINITE norms does not exist in f32 either: the largest finite norm is
            sqrtf(FLT_MAX) = 2^64 (1 - 2^-24), whose square is finite (test_value_edges_cpu.py proves both ends).  A norm that IS
            inf, with a finite dot, is what `overflow` has.
  cos_den_clamp (Cosine)    every row is a multiple of one direction u chosen so that dot(u, u) > |u| * |u| in f32: 3 rows
            +2^j u, 4 rows c u with awkward c, the rest -2^j u.  Queries are +-2^j u.  |sim| rounds above 1 and is clamped: a
            query along +u gets 0.0 three times, up to four awkward values, then exactly 2.0 ordered by id; a query along -u
            gets one tie group at exactly 0.0.
  dot_zero  (Dot)           queries live on the first half of the coordinates (non-negative).  4 rows have a tiny positive dot
            (negative subnormal distances, first), 60 % are orthogonal by disjoint support or have products that underflow to
            +-0 (the fold starts at +0.0, so the dot is +0.0 and the distance -0.0: one tie group, ids decide), the rest have
            tiny or ordinary negative dots.
  nan_hidden (all metrics)  gaussian rows, row HIDDEN holds one NaN.  Hidden: the oracle succeeds.  Alive and eligible: NaN error.
  tame      (all metrics)   the gaussian control.
"""
import numpy as np

F32 = np.float32
F_FINITE = 5
EUCLID, COSINE, DOT = 0, 1, 2


def HIDDEN(n):
    return n // 3


def dead_rows(n, hide=True):
    """Rows every test tombstones: two of the lowest ids and the last one; with `hide` also the row an error family hides."""
    return np.array([0, 2, n - 1] + ([HIDDEN(n)] if hide else []), dtype=np.int64)


def masked_out(n, hide=True):
    """Rows every id mask of the tests excludes, whatever its selectivity."""
    return np.array([1, 5] + ([HIDDEN(n)] if hide else []), dtype=np.int64)


def live_bytes(n, hide=True):
    live = np.ones(n, dtype=np.uint8)
    live[dead_rows(n, hide)] = 0
    return live


def id_mask(n, selectivity, seed, hide=True):
    """(on bool[n], words uint64[]) of a mask over the ids 0 .. n-1 at about `selectivity`; ids 3, 4, 6, 7 stay eligible."""
    on = np.random.default_rng(seed).random(n) < selectivity
    on[[3, 4, 6, 7]] = True
    on[masked_out(n, hide)] = False
    if not hide:
        on[HIDDEN(n)] = True
    m = np.packbits(on.astype(np.uint8), bitorder="little")
    return on, np.concatenate([m, np.zeros((-len(m)) % 8, dtype=np.uint8)]).view(np.uint64)


def _gauss(rng, n, d):
    return rng.standard_normal((n, d)).astype(F32)


def _spread(rng, n, m, lowest=8):
    """m distinct rows: the `lowest` first ids, the rest anywhere but HIDDEN."""
    rest = np.setdiff1d(np.arange(lowest, n), [HIDDEN(n)])
    return np.concatenate([np.arange(lowest), rng.choice(rest, size=m - lowest, replace=False)])


def _n_special(n):
    return min(max(n // 100, 160), n // 4)


# ------------------------------------------------------------------ the families
def inf_tail(rng, n, d, nq, metric, frac=None):
    """frac: share of rows that carry the +inf (default: all but F_FINITE)."""
    assert metric in (EUCLID, DOT)
    rows, q = _gauss(rng, n, d), _gauss(rng, nq, d)
    if frac is None:
        finite = 8 + rng.choice(n - 8, size=F_FINITE, replace=False)
        finite = finite[finite != HIDDEN(n)]
        bad = np.setdiff1d(np.arange(n), finite)
        col, val = rng.integers(0, d, bad.size), np.inf
    elif metric == EUCLID:                             # row against row (a graph build): inf - inf must not arise, so every
        bad = _spread(rng, n, 2 * d)                   # (column, sign) is used once; +inf - (-inf) is +inf
        assert bad.size <= n * frac
        col, val = np.arange(2 * d) % d, np.where(np.arange(2 * d) < d, np.inf, -np.inf)
    else:                                              # inf * x must have one sign wherever two infinite terms meet
        bad = _spread(rng, n, max(int(n * frac), 9))
        rows[bad] = np.abs(rows[bad])
        col, val = rng.integers(0, d, bad.size), np.inf
    rows[bad, col] = val
    if metric == DOT:                                  # +inf * q must be +inf, never inf - inf or inf * 0
        q = np.abs(q) + F32(0.25)
    return rows, q


def overflow(rng, n, d, nq, metric):
    assert d >= 8
    rows, q = _gauss(rng, n, d), _gauss(rng, nq, d)
    if metric == COSINE:                               # tame rows point away from every query: distance > 1
        rows, q = -np.abs(rows) - F32(0.1), np.abs(q) + F32(0.1)
    big = _spread(rng, n, _n_special(n))
    a, b = big[0::2], big[1::2]                        # a: ~3e19, a square overflows; b: ~2e38, a sum of two overflows
    q[:, :4] = rng.uniform(0.5, 1.0, (nq, 4)).astype(F32)
    if metric == COSINE:
        q[:, :4] = rng.uniform(0.25, 0.5, (nq, 4)).astype(F32)
        rows[a[:, None], np.arange(4)] = rng.uniform(2.5e19, 3.5e19, (a.size, 4)).astype(F32)
        rows[b, 0] = rng.uniform(1.5e38, 2.5e38, b.size).astype(F32)          # one element: the dot stays finite
        q[0, d - 4:] = rng.uniform(2.5e19, 3.5e19, 4).astype(F32)             # the rows are tame there: the dot stays finite
    else:
        rows[a[:, None], np.arange(4)] = rng.uniform(2.5e19, 3.5e19, (a.size, 4)).astype(F32)
        rows[b[:, None], np.arange(4)] = rng.uniform(1.5e38, 2.5e38, (b.size, 4)).astype(F32)
        if metric == DOT:                              # all signs equal: +inf meets only finite terms
            q[0, :4] = rng.uniform(2.5e19, 3.5e19, 4).astype(F32)
            q[0] = np.abs(q[0])
            rows[big] = np.abs(rows[big])
            rows[:, :4] = np.abs(rows[:, :4])          # row against row (a graph build) too: no +inf and -inf in one fold
        else:                                          # every row is tame there: every difference squares to inf
            q[0, d - 4:] = rng.uniform(2.5e19, 3.5e19, 4).astype(F32)
    return rows, q


def _small_ints(rng, shape, scale):
    m = rng.integers(-3, 4, shape)
    m[..., 0] = np.where(m[..., 0] == 0, 1, m[..., 0])            # never a zero vector
    return (m * scale).astype(F32)


def subnormal(rng, n, d, nq, metric):
    assert metric in (EUCLID, DOT)
    q = _gauss(rng, nq, d)
    if metric == EUCLID:
        rows = _gauss(rng, n, d) * F32(3.0)            # the ordinary half lies farther from every query than the origin does
        tiny = np.union1d(np.arange(8), np.nonzero(rng.random(n) < 0.5)[0])
        rows[tiny] = _small_ints(rng, (tiny.size, d), 1e-23)
        q[0::2] = _small_ints(rng, (q[0::2].shape[0], d), 1e-23)
        dup = tiny[8:8 + 40]
        rows[dup] = q[0]                               # exact 0.0 distances for query 0, more than any k's worth elsewhere
    else:
        rows = _small_ints(rng, (n, d), 1e-22)
        q[0::2] = _small_ints(rng, (q[0::2].shape[0], d), 1e-22)
    return rows, q


def cos_den_tiny(rng, n, d, nq, metric):
    assert metric == COSINE
    rows, q = _gauss(rng, n, d), _gauss(rng, nq, d)
    tiny = np.union1d(np.arange(8), np.nonzero(rng.random(n) < 0.5)[0])
    mq = _small_ints(rng, (q[0::2].shape[0], d), 1.0)             # the tiny rows lie along the tiny queries, up to one step
    m = mq[rng.integers(0, mq.shape[0], tiny.size)]               # in up to two coordinates: the top-k is theirs, with duplicates
    for _ in range(2):
        m[np.arange(tiny.size), rng.integers(1, d, tiny.size)] += rng.integers(-1, 2, tiny.size).astype(F32)
    m[:8] = mq[0]
    rows[tiny] = (m * 5e-23).astype(F32)
    q[0::2] = (mq * 1e-20).astype(F32)
    return rows, q


def cos_den_zero(rng, n, d, nq, metric):
    assert metric == COSINE
    rows, q = _gauss(rng, n, d), _gauss(rng, nq, d)
    rows[HIDDEN(n)] = F32(1e-25)
    return rows, q


def fltmax_pair():
    """(a, b) with fl(fl(a*a) + fl(b*b)) == FLT_MAX: the vector of the largest finite norm (tests/test_value_edges_cpu.py)."""
    fmax = np.finfo(F32).max
    a = F32(1.5 * 2.0 ** 63)                                       # a*a = 1.125 * 2^127, exact
    b0 = np.sqrt(np.float64(fmax) - np.float64(a) ** 2)
    with np.errstate(over="ignore"):
        for a_ in a + np.arange(0, 4096, dtype=np.float64) * 2.0 ** 40:
            a_ = F32(a_)
            b0 = F32(np.sqrt(np.float64(fmax) - np.float64(a_) ** 2))
            for step in range(-4, 5):
                b_ = F32(np.float64(b0) + step * 2.0 ** 40)
                if F32(F32(a_ * a_) + F32(b_ * b_)) == fmax:
                    return a_, b_
    raise AssertionError("no pair found")


def _fold(x):
    s = F32(0.0)
    for v in x:
        s = F32(s + F32(v * v))
    return s


def clamp_direction(rng, d):
    """u with dot(u, u) strictly above |u| * |u| in the oracle's arithmetic: sim of u with +-2^j u is +-(1 + 2^-23) before the clamp."""
    while True:
        u = (rng.standard_normal(d) * 1.7).astype(F32)
        s = _fold(u)
        nrm = F32(np.sqrt(s))
        if F32(nrm * nrm) < s:
            return u


def cos_den_clamp(rng, n, d, nq, metric):
    assert metric == COSINE
    u = clamp_direction(rng, d)
    pw = (2.0 ** rng.integers(-8, 9, n)).astype(F32)
    rows = -pw[:, None] * u[None, :]
    pos = np.array([3, 4, n // 2])
    rows[pos] = -rows[pos]
    awk = np.array([6, 7, n // 2 + 1, n // 2 + 2])
    rows[awk] = (np.array([7.3, -5.1, 1 / 3, 0.77], dtype=F32)[:, None] * u[None, :]).astype(F32)
    qs = (2.0 ** rng.integers(-4, 5, nq)).astype(F32)
    qs[1::2] = -qs[1::2]
    return rows.astype(F32), (qs[:, None] * u[None, :]).astype(F32)


def dot_zero(rng, n, d, nq, metric):
    assert metric == DOT and d >= 8
    h = d // 2
    q = np.zeros((nq, d), dtype=F32)
    q[:, :h] = rng.uniform(0.5, 1.5, (nq, h)).astype(F32)
    q[0::2, :h] *= F32(1e-20)                                      # tiny queries: their products with 1e-30 underflow
    rows = np.zeros((n, d), dtype=F32)
    kind = rng.random(n)
    kind[:8] = 0.0
    kind[HIDDEN(n)] = 0.0
    orth = kind < 0.45
    rows[orth, h:] = _gauss(rng, int(orth.sum()), d - h)           # disjoint support: every product is +-0
    under = (kind >= 0.45) & (kind < 0.6)                          # +-1e-30 * 1e-20 underflows to +-0; for tame queries a tiny dot
    rows[under, :h] = (rng.choice([-1.0, 1.0], (int(under.sum()), h)) * 1e-30).astype(F32)
    tneg = (kind >= 0.6) & (kind < 0.75)                           # tiny negative dots
    rows[tneg, :h] = -rng.uniform(1e-25, 2e-25, (int(tneg.sum()), h)).astype(F32)
    rest = kind >= 0.75
    rows[rest] = _gauss(rng, int(rest.sum()), d)
    rows[rest, :h] = -np.abs(rows[rest, :h])                       # ordinary negative dots
    tpos = 8 + rng.choice(n - 8, size=4, replace=False)
    tpos = tpos[tpos != HIDDEN(n)]
    rows[tpos] = 0.0
    rows[tpos, :h] = rng.uniform(1e-25, 2e-25, (tpos.size, h)).astype(F32)
    return rows, q


def nan_hidden(rng, n, d, nq, metric):
    rows, q = _gauss(rng, n, d), _gauss(rng, nq, d)
    rows[HIDDEN(n), d // 2] = np.nan
    return rows, q


def tame(rng, n, d, nq, metric):
    return _gauss(rng, n, d), _gauss(rng, nq, d)


ALL = (EUCLID, COSINE, DOT)
FAMILIES = {                                                       # name: (generator, metrics, the oracle's error while HIDDEN is alive)
    "inf_tail": (inf_tail, (EUCLID, DOT), None),
    "overflow": (overflow, ALL, None),
    "subnormal": (subnormal, (EUCLID, DOT), None),
    "cos_den_tiny": (cos_den_tiny, (COSINE,), None),
    "cos_den_clamp": (cos_den_clamp, (COSINE,), None),
    "dot_zero": (dot_zero, (DOT,), None),
    "cos_den_zero": (cos_den_zero, (COSINE,), "InvalidVector"),
    "nan_hidden": (nan_hidden, ALL, "NanDistance"),
    "tame": (tame, ALL, None),
}
ERROR_FAMILIES = tuple(f for f, v in FAMILIES.items() if v[2])
CASES = [(f, m) for f, v in FAMILIES.items() for m in v[1]]         # every (family, metric) the tests run
CASE_IDS = ["%s-m%d" % c for c in CASES]

_CACHE = {}


def make(family, n, d, nq, metric, **kw):
    """The family's rows and queries from a seed fixed by its name and shape; computed once, never written to."""
    key = (family, n, d, nq, metric, tuple(sorted(kw.items())))
    if key not in _CACHE:
        seed = [sum(family.encode()), n, d, nq, metric]
        rows, q = FAMILIES[family][0](np.random.default_rng(seed), n, d, nq, metric, **kw)
        rows, q = np.ascontiguousarray(rows, dtype=F32), np.ascontiguousarray(q, dtype=F32)
        rows.setflags(write=False)
        q.setflags(write=False)
        _CACHE[key] = rows, q
    return _CACHE[key]


# ------------------------------------------------------------------ the two generators tools/fuzz_parity.py draws from
def fuzz_rows(rng, n, d, kind):
    """kind 'overflow' / 'subnormal' as one block of rows or queries for the soak (any metric, any shape): gaussian rows of
    which about 1 % carry one element whose square overflows (its products with gaussian queries stay finite, so no NaN
    arises), or rows of which half are at the bottom of f32."""
    x = _gauss(rng, n, d)
    pick = rng.random(n) < (0.01 if kind == "overflow" else 0.5)
    m = int(pick.sum())
    if kind == "overflow":
        x[pick, 0] = np.abs(x[pick, 0]) * rng.choice([3e19, 1e37], m).astype(F32)
    elif kind == "subnormal":
        x[pick] = _small_ints(rng, (m, d), 1e-22)
    else:
        raise ValueError(kind)
    return x


# ------------------------------------------------------------------ the shapes both test files use: name -> (n, d, nq, ks)
K_LARGE = 113
SHAPES = {
    "direct": (3000, 33, 4, (10, 64)),                             # the direct exact scan of small indexes
    "tiered": (20000, 64, 24, (10,)),                              # above the direct path's row limit; d = 64: the shadow kernel can run
    "ragged": (20000, 33, 24, (10,)),                              # a ragged K stage
    "screened": (65536, 64, 24, (10,)),                            # the fewest rows the bf16 screening tier takes (BF16_MIN_ROWS)
    "wide": (65536, 64, 300, (10,)),                               # the 512-query kernel of the screening tier
}


def large_k_shape(min_rows):
    """min_rows = vdb_flat_large_k_min_rows(K_LARGE), rounded up to whole 512-row blocks."""
    return ((int(min_rows) + 511) // 512 * 512, 32, 8, (K_LARGE,))


def checked_queries(nq):
    """The fixed subset of queries compared with the oracle: the first four (one of every kind a family makes) and the last."""
    return sorted(set(range(min(nq, 4))) | {nq - 1})


def short_mask(n):
    """A mask under which fewer rows are eligible than any k of the tests, two in each third of the index."""
    on = np.zeros(n, dtype=bool)
    on[[3, 4, n // 2, n // 2 + 1, n - 5, n - 4]] = True
    m = np.packbits(on.astype(np.uint8), bitorder="little")
    return on, np.concatenate([m, np.zeros((-len(m)) % 8, dtype=np.uint8)]).view(np.uint64)


# ------------------------------------------------------------------ HNSW: no NaN may arise between two ROWS either
HNSW_SHAPES = [(300, 8), (1500, 48)]
HNSW_CASES = [("overflow", EUCLID), ("overflow", DOT), ("subnormal", EUCLID), ("subnormal", DOT), ("dot_zero", DOT),
              ("inf_tail", EUCLID), ("inf_tail", DOT)]            # overflow under Cosine is inf / inf between two large rows
HNSW_NQ = 12


def make_hnsw(family, n, d, metric):
    return make(family, n, d, HNSW_NQ, metric, **({"frac": 0.10} if family == "inf_tail" else {}))


# ------------------------------------------------------------------ hand-built parts for the merge kernels
MERGE_SHAPES = [(4, 64), (8, 300)]                                 # the LDS sort; the binary-search placement
MERGE_VALUES = np.array([0xff800000, 0xbfc00000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x00011111, 0x3f000000,
                         0x7f800000], dtype=np.uint32).view(F32)   # -inf -1.5 -2^-149 -0.0 +0.0 2^-149 a larger subnormal 0.5 +inf


def merge_order(ids, dists):
    """(distance compared as floats -- so -0.0 == +0.0, as the oracle's cmp_pair has it -- then unsigned id), from numpy alone."""
    return np.lexsort((np.asarray(ids, dtype=np.uint64), np.asarray(dists, dtype=F32)))


def merge_parts(W, B, k, seed):
    """W sorted parts of B queries: (ids u64[W, B, k], dists f32[W, B, k], counts i32[W, B]), some parts short or empty."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(W * B * k).astype(np.uint64).reshape(W, B, k)
    d = MERGE_VALUES[rng.integers(0, MERGE_VALUES.size, (W, B, k))]
    counts = rng.integers(k // 2, k + 1, (W, B)).astype(np.int32)
    counts[1, 0], counts[2, 0], counts[0, 1], counts[3, 2] = 1, 0, k, 0
    for p in range(W):
        for b in range(B):
            o = merge_order(ids[p, b], d[p, b])
            ids[p, b], d[p, b] = ids[p, b][o], d[p, b][o]
    return ids, d, counts

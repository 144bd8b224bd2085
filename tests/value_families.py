"""Value families for the tests at the edges of f32 (tests/test_value_edges_cpu.py, tests/test_gpu_value_edges.py, and, for the
reads by stored id, recommend, one row per group, a filter per query and MMR, tests/test_gpu_value_edges_reads.py: the additions
at the end of this file).

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
  bf16_edge (all metrics)   finite elements whose bf16 piece is not: about 1 % of the rows (at least 160) hold in column 0 one of
            +-0x7f7f7fff (the bf16 piece stays finite), +-0x7f7f8000 (the tie) and +-0x7f7fffff (both round to the bf16 infinity,
            by round-to-nearest-even and in the hi word of the SPLIT layout alike), or 0x00007fff, 0x00008000, 0x007f8000 (the bf16
            piece is 0, the smallest subnormal, the smallest normal number); their other elements are ordinary ties.  Euclid: such a
            row is +inf away (the square overflows), the top-k is tame.  Dot: the products stay finite, the rows with +FLT_MAX lead
            with one distance near -2.5e38, ids decide, then the two patterns next to the tie.  Cosine: the row norm is inf and the
            dot finite, the distance exactly 1.0, the tame rows point away: the 1.0 group, ids decide.  No NaN, no error.
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


# the magnitudes bf16_edge puts into column 0, as f32 bit patterns, and what the hi word of the SPLIT layout (upper half + bit 15)
# and round-to-nearest-even make of each
BF16_EDGE_BITS = (0x7f7f7fff,                                      # the last pattern below the tie: hi = 0x7f7f, finite
                  0x7f7f8000,                                      # the tie: hi = 0x7f80, the bf16 infinity, for a finite element
                  0x7f7fffff,                                      # FLT_MAX: hi = 0x7f80
                  0x00007fff,                                      # a subnormal below half the smallest bf16 subnormal: hi = 0
                  0x00008000,                                      # the tie above it: hi = 0x0001, the smallest bf16 subnormal
                  0x007f8000)                                      # the largest f32 subnormals round up to hi = 0x0080, a normal number
BF16_EDGE_LARGE = BF16_EDGE_BITS[:3]


def bf16_edge(rng, n, d, nq, metric):
    """Finite elements at the two ends of what a bf16 word can hold.  About 1 % of the rows (at least 160, rows 0 .. 7 among them)
    are special: column 0 holds one of BF16_EDGE_BITS -- the three large ones with both signs, nine patterns in turn, rows 1, 3,
    4, 6 and 7 all +FLT_MAX -- and every other element of a special row is an ordinary tie (low half 0x8000).  Only column 0 is
    large and the queries are positive and below 1 there, so a product with it stays finite and no fold meets inf - inf."""
    assert d >= 8
    rows, q = _gauss(rng, n, d), _gauss(rng, nq, d)
    if metric == COSINE:                               # tame rows point away from every query: distance > 1 (as in `overflow`)
        rows, q = -np.abs(rows) - F32(0.1), np.abs(q) + F32(0.1)
        rows[:, 0] = -rng.uniform(0.1, 0.9, n).astype(F32)         # ... and stay below 1 in column 0: a stored row that becomes a
    sp = _spread(rng, n, _n_special(n))                            #     query has a finite product with every large element
    bits = rows.view(np.uint32)
    ties = (bits[sp] & np.uint32(0xffff0000)) | np.uint32(0x8000)
    a, b, c = (np.uint32(x) for x in BF16_EDGE_LARGE)
    neg = np.uint32(0x80000000)
    turn = np.array([a, a | neg, b, b | neg, c, c | neg] + list(BF16_EDGE_BITS[3:]), dtype=np.uint32)
    ties[:, 0] = turn[np.arange(sp.size) % turn.size]
    ties[:8, 0] = [a, c, b, c, c, c | neg, c, c]
    bits[sp] = ties
    q[:, 0] = rng.uniform(0.25, 0.5, nq).astype(F32) if metric == COSINE else rng.uniform(0.5, 1.0, nq).astype(F32)
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
    "bf16_edge": (bf16_edge, ALL, None),
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


def large_k_split_shape(min_rows):
    """the large-k shape at d = 64: a row pitch of 32 floats cannot take the SPLIT layout (ld % 64), one of 64 can"""
    n, _, nq, ks = large_k_shape(min_rows)
    return (n, 64, nq, ks)


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


# ------------------------------------------------------------------ reads whose QUERY is built from stored rows (by id, recommend)
# A stored row that becomes a query brings its +-inf, 3e19 or 1e-23 to the query side.  inf_tail in its plain form then puts +inf
# against +inf in one column of nearly every pair (inf - inf under Euclid, and a query that is no longer positive under Dot): those
# stay as ERROR cases; the row-safe form (frac=0.10, what make_hnsw uses) is the one that is answered.  tests/test_value_edges_cpu.py
# pins, id by id, what the oracle answers.
ROW_QUERY_CASES = ([(f, m, {"frac": 0.10} if f == "inf_tail" else {}) for f, m in CASES]
                   + [("inf_tail", m, {}) for m in (EUCLID, DOT)])
ROW_QUERY_IDS = ["%s%s-m%d" % (f, "" if f != "inf_tail" else ("-rowsafe" if kw else "-plain"), m) for f, m, kw in ROW_QUERY_CASES]
READ_SHAPES = ("direct", "tiered")                                 # every read kind; by id and recommend also run "screened"
N_SEEDED = 40


def by_id_ids(n):
    """The stored ids the by-id tests ask about: the low ids every family keeps inside its widest tie group, the rows
    cos_den_clamp makes special, two of short_mask, and 40 seeded live ones."""
    fixed = [1, 3, 4, 6, 7, 8, 9, n // 2, n // 2 + 1, n - 5]
    live = np.setdiff1d(np.arange(n), np.concatenate([dead_rows(n), fixed]))
    more = np.random.default_rng([20291, n]).choice(live, N_SEEDED, replace=False)
    return np.concatenate([fixed, np.sort(more)]).astype(np.int64)


def row_requests(n, count=12):
    """`count` seeded recommend requests over live rows: positives of length 1, 2, 5, 9 (in turn), 0 - 2 negatives."""
    rng = np.random.default_rng([20292, n])
    live = np.setdiff1d(np.arange(n), dead_rows(n))
    reqs = []
    for b in range(count):
        e = [int(x) for x in rng.choice(live, (1, 2, 5, 9)[b % 4] + (b // 4) % 3, replace=False)]
        cut = (1, 2, 5, 9)[b % 4]
        reqs.append((tuple(e[:cut]), tuple(e[cut:])))
    reqs[3] = (reqs[3][0][:8] + (1,), reqs[3][1])                  # a row of every family's tie group among nine positives
    return tuple(reqs)


# ------------------------------------------------------------------ the recommend fold at the edges of f32
FOLD_N = 64
FOLD_COLS = {"subnormal": 0, "zero": 1, "overflow": 2, "inf_minus_inf": 3, "fltmax": 4, "cancel": 5}
FOLD_FIRST_TAME = 6                                                # columns 6 .. d-1 are gaussian in every ordinary row
FOLD_REQUESTS = (                                                  # (name, positives, negatives)
    ("subnormal_5", (8, 9, 10, 11, 12), ()),                      # sp = a multiple of 2^-149 near 2^-128; sp * 0.2f rounds inside the subnormal range
    ("subnormal_9_2", (8, 9, 10, 11, 12, 13, 14, 15, 16), (44, 45)),
    ("cancel_to_plus_zero", (19,), (20,)),                         # equal rows: ap - an = +0.0 in every element
    ("minus_zero", (17,), (18,)),                                  # -0.0 + (-0.0 - +0.0) = -0.0
    ("overflow_mid_fold", (22, 23, 24, 25, 46), ()),               # 2e38 + 2e38 = inf, then -2e38, -2e38: the average is finite, the fold is inf
    ("inf_minus_inf", (26, 27), (28, 29)),                         # ap = an = inf: NaN, an error under every metric
    ("fltmax_times_rp", (30, 31, 47), ()),                         # FLT_MAX * fl(1 / 3)
    ("cosine_norm_underflows", (32, 33), ()),                      # 1e-25 everywhere, +1 and -1 cancel: not all zero, norm 0
    ("tame_9_5", (48, 49, 50, 51, 52, 53, 54, 55, 56), (57, 58, 59, 60, 61)),
    ("tame_2_9", (62, 48, ), (49, 50, 51, 52, 53, 54, 55, 56, 57)),
    ("tame_1_2", (58,), (59, 60)),
    ("tame_5_1", (34, 62, 3, 37, 35), (39,)),                      # rows of all three shards of a sharded handle, not in their order
)
# what the oracle answers for the folds (pinned by tests/test_value_edges_cpu.py): request name -> {metric: error}
FOLD_ERRORS = {
    "inf_minus_inf": {EUCLID: "NanDistance", COSINE: "NanDistance", DOT: "NanDistance"},
    "cosine_norm_underflows": {COSINE: "InvalidVector"},
    "overflow_mid_fold": {COSINE: "NanDistance"},                  # the norm of the fold is inf and so is its dot with every row: inf / inf
    "fltmax_times_rp": {COSINE: "NanDistance"},                    # likewise against the FLT_MAX row itself
}


def fold_edges(d):
    """(rows f32[64, d], requests): a hand-built block for the recommend fold (include/vdb_flat.h: a left fold from the first row,
    one multiply by fl(1 / n), ap + (ap - an)).  Every phenomenon lives in a column of its own (FOLD_COLS), so that no distance
    becomes NaN unless the request is an intended error (FOLD_ERRORS); the rows dead_rows(64) tombstones hold nothing special.
      column 0   rows 8 .. 16 hold (2^19 + odd) * 2^-149: subnormal, their sums and averages stay subnormal.  Rows 40 .. 43 hold
                 +-2^127 there and point along the fold of rows 8 .. 16 elsewhere: under Dot they lead its list and
                 subnormal * 2^127 is an ordinary number, so a flushed fold changes their distance bits.
      column 1   row 17 holds -0.0, row 18 +0.0
      column 2   1.0 in every row (the fold of "overflow_mid_fold" is +inf there: inf * 0 must not arise), 1e-25 in rows 32, 33;
                 rows 22, 23 hold 2e38 and rows 24, 25 -2e38
      column 3   rows 26 .. 29 hold 3e38: two of them fold to inf on either side
      column 4   row 30 holds FLT_MAX
      rows 19, 20 are equal; rows 32, 33 hold 1e-25 everywhere but +1 / -1 in column 5."""
    assert d >= 32
    key = ("fold_edges", d)
    if key not in _CACHE:
        rng = np.random.default_rng([20293, d])
        rows = _gauss(rng, FOLD_N, d)
        c = FOLD_COLS
        rows[:, :FOLD_FIRST_TAME] = 0.0
        rows[:, c["overflow"]] = 1.0
        sub = np.arange(8, 17)
        rows[sub, c["subnormal"]] = ((2 ** 19 + 2 * np.arange(9) + 1) * 2.0 ** -149).astype(F32)
        lead = np.arange(40, 44)
        rows[lead] = F32(2.0) * rows[sub].mean(0, dtype=F32) + F32(0.05) * _gauss(rng, 4, d)
        rows[lead, :FOLD_FIRST_TAME] = 0.0
        rows[lead, c["overflow"]] = 1.0
        rows[lead, c["subnormal"]] = np.array([1, -1, 1, -1], dtype=F32) * F32(2.0 ** 127)
        rows[17, c["zero"]] = F32(-0.0)
        rows[20] = rows[19]
        rows[[22, 23], c["overflow"]] = F32(2e38)
        rows[[24, 25], c["overflow"]] = F32(-2e38)
        rows[26:30, c["inf_minus_inf"]] = F32(3e38)
        rows[30, c["fltmax"]] = np.finfo(F32).max
        rows[[32, 33]] = F32(1e-25)
        rows[32, c["cancel"]], rows[33, c["cancel"]] = F32(1.0), F32(-1.0)
        used = np.concatenate([lead] + [np.array(p + n) for _, p, n in FOLD_REQUESTS])
        assert not np.isin(dead_rows(FOLD_N), used).any()
        rows = np.ascontiguousarray(rows, dtype=F32)
        rows.setflags(write=False)
        _CACHE[key] = rows
    return _CACHE[key], tuple((p, n) for _, p, n in FOLD_REQUESTS)


# ------------------------------------------------------------------ one row per group: codes that need stage A, B and C
DISTINCT_KS = {"A": 3, "B": 8, "C": 16}
DISTINCT_GIANT = 7


def distinct_codes(family, metric, n, d, nq, **kw):
    """i32[n]: a code column laid along the ORACLE's ranking of query 0 over the live rows (rank position p), the giant_codes idea
    of distinct_data: the rows at p = 3 .. 199 and 210 .. 1499 share one code.  Where the family's tie group leads the ranking
    these are its lowest ids, and the group's representative is decided by id alone.  p = 0, 2 and 200 .. 209 have codes of their
    own, p = 1 has none (-1: a group of its own); behind p = 1500 a row has code 100 + p % 500, every 97th none.  Query 0 then
    sees 4 groups in its first 32 / 64 ranks and 14 in its first 1024: k = 3 ends in stage A, k = 8 in stage B, k = 16 in stage C
    (distinct_data.stage_of; tests/test_value_edges_cpu.py asserts it).  Dead rows keep code -1."""
    key = ("distinct_codes", family, metric, n, d, nq, tuple(sorted(kw.items())))
    if key not in _CACHE:
        import oracle
        rows, q = make(family, n, d, nq, metric, **kw)
        oi, _ = oracle.flat_search(metric, rows, q[0], n, live=live_bytes(n))
        p = np.arange(len(oi))
        c = (100 + p % 500).astype(np.int32)
        c[p % 97 == 0] = -1
        c[:1500] = DISTINCT_GIANT
        c[[0, 2]] = [10, 12]
        c[1] = -1
        c[200:210] = 20 + np.arange(10)
        codes = np.full(n, -1, dtype=np.int32)
        codes[oi.astype(np.int64)] = c
        codes.setflags(write=False)
        _CACHE[key] = codes
    return _CACHE[key]


# ------------------------------------------------------------------ one batch, a filter per query: five bindings
GROUP_NONE = 0xFFFFFFFF
GROUP_HOLDS_HIDDEN = 0                                             # with hide=False only this mask (and no mask at all) admits HIDDEN(n)


def group_masks(n, hide=True):
    """(on bool[4, n], words u64[4, (n + 63) // 64], binding): masks 0 .. 3 = about half the ids, about 1 %, short_mask, nothing;
    binding(nq) = u32[nq] binds the queries round-robin to 0, 1, 2, 3, GROUP_NONE.  With hide=False the row HIDDEN(n) is eligible
    under mask 0 alone (and for the unfiltered queries, to whom every live row is)."""
    ons = [id_mask(n, 0.5, 7, hide=hide)[0], id_mask(n, 0.01, 7)[0], short_mask(n)[0], np.zeros(n, dtype=bool)]
    on = np.stack(ons)
    assert not on[1:, HIDDEN(n)].any() and on[0, HIDDEN(n)] == (not hide)
    words = np.zeros((4, (n + 63) // 64), dtype=np.uint64)
    for g in range(4):
        m = np.packbits(on[g].astype(np.uint8), bitorder="little")
        words[g].view(np.uint8)[:m.size] = m

    def binding(nq):
        return np.array([(0, 1, 2, 3, GROUP_NONE)[b % 5] for b in range(nq)], dtype=np.uint32)
    return on, words, binding


def group_queries(q):
    """the grouped batch of a shape: its queries, repeated until every one of the five bindings has at least two"""
    reps = max(1, -(-10 // len(q)))
    return np.ascontiguousarray(np.concatenate([q] * reps)) if reps > 1 else q

"""Data for the certificate tests (test_gpu_certificate.py, test_gpu_certificate_layouts.py, test_certificate_cpu.py): the
adversarial kinds of the first file, the COHERENT families, the two roundings a filter kernel may read a row in, and a
float64 model of score, implied distance and error budget built from the documented formulas alone (DESIGN.md 4.1,
vdb_cert.cpp margin_plan, row_stats_kernel, query_prep).  Needs no device.

Why coherent data.  The certified bound is Cauchy-Schwarz on  dot(q, d) - dot(bf16 q, bf16 d) = e_q.d + bf16(q).e_d.  It is
tight when the rounding errors of a row all point the same way and the query is proportional to them: every element half a
bf16 ulp off in the direction of its sign, the query all ones (or the row's sign pattern).  Rounding half up in magnitude
(row_split.h's hi plane) does that on every row whose low halves are all 0x8000, whatever the upper halves' parity; RNE does
it on low halves that are all 0x7fff or all 0x8001.  Random data never comes near: its errors cancel like a random walk.
"""
import numpy as np

import oracle


def bf16_rne(x):
    """RNE rounding of f32 to bf16 (what v_cvt_pk_bf16_f32 keeps), as f32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_half_up(x):
    """row_split.h's hi piece of f32 (upper half + bit 15: rounded half up in magnitude), as f32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (((b >> 16) + ((b >> 15) & 1)) & 0xFFFF) << 16
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_truncate(x):
    """The upper half alone: what a WRONG layout codec would hand the kernel (the mutant the coherent families must catch)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return b.view(np.float32).reshape(np.shape(x))


def make_case(kind, metric, rng, d=None):
    """(rows, queries): adversarial for the error bound.  d: another dimension than the kind's own."""
    if kind == "cancel":
        # heavy cancellation: alternating signs, every dot product is a difference of two large nearly equal sums
        n, d, nq = 66_000, d or 96, 48
        base = rng.random((n, d), dtype=np.float32) + 0.5
        sign = np.where(np.arange(d) % 2 == 0, 1.0, -1.0).astype(np.float32)
        rows = base * sign
        q = (rng.random((nq, d), dtype=np.float32) + 0.5) * sign * np.where(rng.random((nq, 1)) < 0.5, 1, -1).astype(np.float32)
        q[: nq // 2] = np.abs(q[: nq // 2])                      # these cancel against the rows' signs
    elif kind == "scales":
        # magnitudes from 1e-21 to 1e+17 between rows AND inside a row (1e18 squared times the dimension overflows f32)
        n, d, nq = 66_100, d or 64, 48
        top = 17.0                                               # |d|^2 (and Euclid's |d|^2 + 2|q||d|) must stay finite in f32
        rexp = rng.uniform(-18, top, (n, 1))
        rows = (rng.standard_normal((n, d)) * 10.0 ** (rexp + rng.uniform(-3, 0, (n, d)))).astype(np.float32)
        qexp = rng.uniform(-18, top, (nq, 1))
        q = (rng.standard_normal((nq, d)) * 10.0 ** (qexp + rng.uniform(-3, 0, (nq, d)))).astype(np.float32)
    elif kind == "dim16384":
        n, d, nq = 1_500, d or 16384, 8
        rows = rng.standard_normal((n, d)).astype(np.float32)
        q = rng.standard_normal((nq, d)).astype(np.float32)
        q[0] = rows[7] + 1e-4 * rng.standard_normal(d).astype(np.float32)
    elif kind == "bf16ties":
        # clusters whose bf16 images collide: perturbations far below the bf16 resolution of the values
        n, d, nq = 65_800, d or 128, 32
        centres = rng.standard_normal((n // 200 + 1, d)).astype(np.float32)
        rows = (centres[np.arange(n) // 200] * (1.0 + 2e-5 * rng.standard_normal((n, d)))).astype(np.float32)
        q = (centres[rng.integers(0, centres.shape[0], nq)] * (1.0 + 1e-5 * rng.standard_normal((nq, d)))).astype(np.float32)
    elif kind == "subnormal":
        # f32 subnormals (below 1.18e-38) and values whose products underflow
        n, d, nq = 65_700, d or 40, 24
        rows = (rng.standard_normal((n, d)) * 10.0 ** rng.uniform(-41, -17, (n, 1))).astype(np.float32)
        q = (rng.standard_normal((nq, d)) * 10.0 ** rng.uniform(-24, -15, (nq, 1))).astype(np.float32)
        q[::2] = (rng.standard_normal((nq // 2, d)) * 10.0 ** rng.uniform(-6, 2, (nq // 2, 1))).astype(np.float32)   # ordinary queries against tiny rows
        rows[:8] = (rng.standard_normal((8, d)) * 1e-3).astype(np.float32)   # a few ordinary rows keep Cosine defined
    else:
        raise ValueError(kind)
    if metric == 1:
        rows[np.linalg.norm(rows.astype(np.float64), axis=1) == 0] = 1.0
        bad = ~np.isfinite(np.linalg.norm(rows.astype(np.float64), axis=1).astype(np.float32)) | \
            (np.sqrt((rows.astype(np.float32) ** 2).sum(1)) == 0)
        rows[bad] = 1.0                                         # a zero (or f32-underflowing) norm fails every Cosine search
        qb = np.sqrt((q.astype(np.float32) ** 2).sum(1)) == 0
        q[qb] = 1.0
    return rows, q


def exact_distances(metric, rows, q):
    """Oracle distances of every row (f32 bits of the reference's arithmetic), as [n] f32, via one full-k search."""
    n = rows.shape[0]
    ids, d = oracle.flat_search(metric, rows, q, n)
    out = np.empty(n, dtype=np.float32)
    out[ids.astype(np.int64)] = d
    return out


# ------------------------------------------------------------------ coherent families
# family -> (low half of every element, parity of the upper half: 0 even, 1 odd, None as drawn)
FAMILIES = {
    "below": (0x7FFF, None),           # just under the tie: both roundings go down by (almost) half an ulp
    "tie_even": (0x8000, 0),           # the tie, even upper half: RNE goes down, hi goes up
    "tie_odd": (0x8000, 1),            # the tie, odd upper half: both go up
    "tie_mixed": (0x8000, None),       # the tie, parity as drawn: RNE's errors cancel, hi's do not
    "above": (0x8001, None),           # just over the tie: both go up by (almost) half an ulp
    "three_quarter": (0xC000, None),   # both go up by a quarter ulp; a codec that truncates is off by three quarters
}
COHERENT_QUERIES = 16


def _forced(rng, shape, low, parity):
    """f32 in [1, 2) with the low half (and the upper half's parity) forced"""
    b = (rng.random(shape, dtype=np.float32) + np.float32(1.0)).view(np.uint32)
    b = (b & np.uint32(0xFFFF0000)) | np.uint32(low)
    if parity is not None:
        b = (b & np.uint32(0xFFFEFFFF)) | np.uint32(parity << 16)
    return b.view(np.float32)


def coherent(family, metric, d, n, rng):
    """(rows [n, d], queries [16, d], pattern [d]): every row element has the family's low half; the rows' exponents run from
    2^-20 to 2^20 (one per row: powers of two and signs leave the low halves alone, Euclid stays finite), the odd rows carry one
    +-1 pattern.  Queries: all ones, the pattern, bf16-exact multiples of both, two all-tie queries (odd upper halves; even
    ones under the pattern), two proportional to stored rows, the rest gaussian."""
    low, parity = FAMILIES[family]
    pattern = np.where(rng.random(d) < 0.5, -1.0, 1.0).astype(np.float32)
    rows = _forced(rng, (n, d), low, parity)
    rows *= np.exp2(rng.integers(-20, 21, (n, 1))).astype(np.float32)
    rows[1::2] *= pattern
    q = rng.standard_normal((COHERENT_QUERIES, d)).astype(np.float32)
    ones = np.ones(d, dtype=np.float32)
    q[0], q[1] = ones, pattern
    q[2], q[3] = np.float32(3.0) * ones, np.float32(0.375) * pattern
    q[4] = _forced(rng, d, 0x8000, 1)
    q[5] = _forced(rng, d, 0x8000, 0) * pattern
    q[6] = rows[n // 3 & ~1] * np.float32(2.0)                   # a row without the pattern, a row with it
    q[7] = rows[(2 * n // 3) | 1] * np.float32(0.25)
    return np.ascontiguousarray(rows), np.ascontiguousarray(q), pattern


def tie_free(d, n, nq, rng):
    """Plain data WITHOUT a tie element: gaussian rows x row scales 0.1 .. 4, bit 0 flipped wherever a low half is 0x8000 --
    the two roundings then agree on every element."""
    rows = rng.standard_normal((n, d), dtype=np.float32) * rng.uniform(0.1, 4.0, (n, 1)).astype(np.float32)
    b = rows.view(np.uint32)
    b[(b & np.uint32(0xFFFF)) == 0x8000] ^= np.uint32(1)
    return rows, rng.standard_normal((nq, d), dtype=np.float32)


# ------------------------------------------------------------------ the float64 model
def cert_constants(metric, d):
    """eps_coef, c_acc and the margin plan as vdb_cert.cpp computes them (f32 where the library stores f32)."""
    ld = -(-d // 32) * 32
    u = 2.0 ** -24
    eps = float(np.float32(1.1 * {0: ld + 4.0, 1: 2.0 * ld + 16.0, 2: 2.0 * ld + 2.0}[metric] * u))
    c_acc = float(np.float32(ld * 2.0 ** -22 * 1.05))
    two = 2.0 if metric == 0 else 1.0
    Ae, An, Bn = two * 1.01 * 1.004, two * (c_acc + eps), two * 1.01
    kappa = Bn / (Ae * 1.0e-3 + An)
    f = lambda v: float(np.float32(v))
    return {"ld": ld, "eps": eps, "c_acc": c_acc, "m_e": f(Ae), "m_n": f(An * 1.000001), "m_b": f(Bn / kappa * 1.000001), "kappa": f(kappa * 1.000001)}


def model_ratios(metric, rows, q, round_rows):
    """[nq, n] error / budget in float64: the score of EXACT arithmetic on bf16_rne(q) and round_rows(rows) against the exact
    distance, over the budget the certificate grants (the (B) formulas of test_gpu_certificate.py with every quantity from
    its documented definition: margins and rho from the RNE error of the rows, as row_stats_kernel computes them whatever
    the layout).  What the real kernel and the oracle add in f32 is covered by the (c_acc + eps) |q||d| share of that budget."""
    c = cert_constants(metric, rows.shape[1])
    eps, c_acc, ld = c["eps"], c["c_acc"], c["ld"]
    R, Q = rows.astype(np.float64), q.astype(np.float64)
    Qb = bf16_rne(q).astype(np.float64)
    acc = Qb @ round_rows(rows).astype(np.float64).T
    nd, ed = np.linalg.norm(R, axis=1), np.linalg.norm(R - bf16_rne(rows).astype(np.float64), axis=1)
    qn = np.linalg.norm(Q, axis=1)[:, None]
    eq = np.linalg.norm(Q - Qb, axis=1)[:, None] * (1.0001 + ld * 1.0e-7)                        # query_prep's slack
    g = (qn * (1.00001 + ld * 1.2e-7) + c["kappa"] * eq) * 1.00001
    margin = np.maximum(c["m_e"] * ed + c["m_n"] * nd, c["m_b"] * nd) * 1.000001
    dot = Q @ R.T
    if metric == 2:
        err, budget = np.abs(-acc + dot), g * margin
    elif metric == 0:
        d2 = np.stack([((R - Q[b]) ** 2).sum(1) for b in range(len(Q))])
        err = np.abs(nd * nd * (1.0 - eps) - 2.0 * acc + qn * qn - d2)
        budget = g * margin + eps * nd * nd + eps * (qn * qn + d2)
    else:
        err = np.abs((1.0 - acc / (nd * qn)) - (1.0 - dot / (nd * qn)))
        budget = 1.01 * (eq / qn + 1.004 * float(np.max(ed / nd))) + c_acc + eps + 0.0 * err
    return err / budget

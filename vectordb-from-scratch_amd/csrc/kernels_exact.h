// kernels_exact.h -- the device functions that more than one translation unit of kernels needs: the reference's exact-order
// arithmetic (src/distance.rs:37-73, src/vector.rs:35-37) and the screening tier's certificate with its inverse, the score
// cut.  Every includer is built with -ffp-contract=off: each multiply and add below rounds on its own.
#pragma once
#include "kernels.h"

#pragma clang fp contract(off)

namespace vdb {

// ---------------------------------------------------------------------------------------------
// Exact-order arithmetic: sequential f32 left folds, one rounding per operation.
// sqrt uses __builtin_sqrtf (correctly rounded expansion); HIP's __fsqrt_rn lowers to a bare
// v_sqrt_f32 (1 ulp) on gfx950 and is NOT usable for bit parity.
// ---------------------------------------------------------------------------------------------
// Each fold loads 16 elements (4 x 16 bytes) before it consumes them, so the loads of a block are in
// flight together while the adds stay one strictly sequential chain.
__device__ __forceinline__ float fold_sq(const float* __restrict__ x, uint32_t d) {
    // vector.rs:35-37   sum_i x_i*x_i
    float s = 0.0f;
    uint32_t i = 0;
    for (; i + 16 <= d; i += 16) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(x + i + 4 * u);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s = __fadd_rn(s, __fmul_rn(v[u].x, v[u].x));
            s = __fadd_rn(s, __fmul_rn(v[u].y, v[u].y));
            s = __fadd_rn(s, __fmul_rn(v[u].z, v[u].z));
            s = __fadd_rn(s, __fmul_rn(v[u].w, v[u].w));
        }
    }
    for (; i < d; ++i) s = __fadd_rn(s, __fmul_rn(x[i], x[i]));
    return s;
}

__device__ __forceinline__ float fold_dot(const float* __restrict__ q, const float* __restrict__ x, uint32_t d) {
    // distance.rs:67-73   sum_i a_i*b_i
    float s = 0.0f;
    uint32_t i = 0;
    for (; i + 16 <= d; i += 16) {
        float4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = *reinterpret_cast<const float4*>(q + i + 4 * u);
            b[u] = *reinterpret_cast<const float4*>(x + i + 4 * u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s = __fadd_rn(s, __fmul_rn(a[u].x, b[u].x));
            s = __fadd_rn(s, __fmul_rn(a[u].y, b[u].y));
            s = __fadd_rn(s, __fmul_rn(a[u].z, b[u].z));
            s = __fadd_rn(s, __fmul_rn(a[u].w, b[u].w));
        }
    }
    for (; i < d; ++i) s = __fadd_rn(s, __fmul_rn(q[i], x[i]));
    return s;
}

__device__ __forceinline__ float fold_sqdiff(const float* __restrict__ q, const float* __restrict__ x, uint32_t d) {
    // distance.rs:37-44   sum_i (a_i-b_i)^2   (powi(2) == t*t)
    float s = 0.0f;
    uint32_t i = 0;
    for (; i + 16 <= d; i += 16) {
        float4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = *reinterpret_cast<const float4*>(q + i + 4 * u);
            b[u] = *reinterpret_cast<const float4*>(x + i + 4 * u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float t;
            t = __fsub_rn(a[u].x, b[u].x); s = __fadd_rn(s, __fmul_rn(t, t));
            t = __fsub_rn(a[u].y, b[u].y); s = __fadd_rn(s, __fmul_rn(t, t));
            t = __fsub_rn(a[u].z, b[u].z); s = __fadd_rn(s, __fmul_rn(t, t));
            t = __fsub_rn(a[u].w, b[u].w); s = __fadd_rn(s, __fmul_rn(t, t));
        }
    }
    for (; i < d; ++i) { float t = __fsub_rn(q[i], x[i]); s = __fadd_rn(s, __fmul_rn(t, t)); }
    return s;
}

// The same folds over a SLICE of the pair, resumed from a partial sum: fold(q, x, d) == part(q + d1, x + d1, d - d1, part(q, x, d1, 0))
// for any d1 that is a multiple of 16 (the same sequence of roundings, element by element) -- rerank_kernel's K slices.
typedef float vdb_f2 __attribute__((ext_vector_type(2)));
// (products and differences two at a time -- v_pk_mul_f32 / v_pk_add_f32, each lane of a packed op rounds exactly like the
// scalar op -- the ADDS stay one by one, in order: the fold is the reference's.  One wave folds 48 candidates and is bound by
// its own instruction stream, so fewer instructions per element is time.)
__device__ __forceinline__ float fold_dot_part(const float* __restrict__ q, const float* __restrict__ x, uint32_t d, float s) {
    uint32_t i = 0;
    for (; i + 16 <= d; i += 16) {
        float4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = *reinterpret_cast<const float4*>(q + i + 4 * u);
            b[u] = *reinterpret_cast<const float4*>(x + i + 4 * u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const vdb_f2 p01 = vdb_f2{a[u].x, a[u].y} * vdb_f2{b[u].x, b[u].y};
            const vdb_f2 p23 = vdb_f2{a[u].z, a[u].w} * vdb_f2{b[u].z, b[u].w};
            s = __fadd_rn(s, p01.x);
            s = __fadd_rn(s, p01.y);
            s = __fadd_rn(s, p23.x);
            s = __fadd_rn(s, p23.y);
        }
    }
    for (; i < d; ++i) s = __fadd_rn(s, __fmul_rn(q[i], x[i]));
    return s;
}
__device__ __forceinline__ float fold_sqdiff_part(const float* __restrict__ q, const float* __restrict__ x, uint32_t d, float s) {
    uint32_t i = 0;
    for (; i + 16 <= d; i += 16) {
        float4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = *reinterpret_cast<const float4*>(q + i + 4 * u);
            b[u] = *reinterpret_cast<const float4*>(x + i + 4 * u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const vdb_f2 t01 = vdb_f2{a[u].x, a[u].y} - vdb_f2{b[u].x, b[u].y};
            const vdb_f2 t23 = vdb_f2{a[u].z, a[u].w} - vdb_f2{b[u].z, b[u].w};
            const vdb_f2 p01 = t01 * t01, p23 = t23 * t23;
            s = __fadd_rn(s, p01.x);
            s = __fadd_rn(s, p01.y);
            s = __fadd_rn(s, p23.x);
            s = __fadd_rn(s, p23.y);
        }
    }
    for (; i < d; ++i) { float t = __fsub_rn(q[i], x[i]); s = __fadd_rn(s, __fmul_rn(t, t)); }
    return s;
}
// the distance from the finished fold (s = sum of squared differences under Euclid, the dot product otherwise)
__device__ __forceinline__ float distance_from_fold(int metric, float s, float qn, float xn) {
    if (metric == EUCLID) return __builtin_sqrtf(s);
    if (metric == DOT) return -s;
    float den = __fmul_rn(qn, xn);                 // norm1 * norm2   distance.rs:58
    float sim = __fdiv_rn(s, den);
    if (sim < -1.0f) sim = -1.0f;                  // f32::clamp keeps NaN
    if (sim > 1.0f) sim = 1.0f;
    return __fsub_rn(1.0f, sim);
}

// DistanceMetric::distance (distance.rs:20-33) for one (query, row) pair.
// qn / xn are the exact-order norms of query and row (only read under Cosine).
__device__ __forceinline__ float exact_distance(int metric, const float* __restrict__ q,
                                                const float* __restrict__ x, uint32_t d, float qn, float xn) {
    if (metric == EUCLID) return __builtin_sqrtf(fold_sqdiff(q, x, d));
    float dot = fold_dot(q, x, d);
    if (metric == DOT) return -dot;
    float den = __fmul_rn(qn, xn);                 // norm1 * norm2   distance.rs:58
    float sim = __fdiv_rn(dot, den);
    if (sim < -1.0f) sim = -1.0f;                  // f32::clamp keeps NaN
    if (sim > 1.0f) sim = 1.0f;
    return __fsub_rn(1.0f, sim);
}

// The certification test: every row not re-ranked has ranking score >= T; is the k-th exact distance ek below the
// lower bound that T implies for such a row's exact distance?  (DESIGN.md "certified top-k")
// UNDERFLOW (found by tests/test_gpu_certificate.py "subnormal"): every bound below takes f32 norms and sums as accurate
// to a few K 2^-24 RELATIVE.  That fails when the squares underflow f32 (|x| below ~1e-19: fold(x*x) loses its low terms
// or all of them), so
//   * a query whose exact-order norm is below 2^-40 is never certified by an MFMA tier (it ends in the exact scan);
//   * under Cosine an index holding a live-or-dead row with 0 < |d| < 2^-40 certifies nothing (same consequence);
//   * every test gives away an ABSOLUTE floor of K 2^-140 in product units for the f32 operations that underflowed
//     along the way (each loses less than 2^-149; the MFMA accumulators themselves keep denormals -- measured).
constexpr double CERT_TINY_NORM = 9.094947017729282e-13;        // 2^-40
__device__ __forceinline__ double cert_floor(const RerankParams& p) { return (double)p.ld * 7.174648137343064e-43; }   // ld 2^-140
// The test has the form   lhs(e_k) < a + b * (T - |T| tslack)   with lhs = e_k, or e_k^2 (1 + eps) under Euclid.  a, b and
// tslack depend on the QUERY only (norms, rounding-error norm, per-index scalars): they are computed once per workgroup --
// double-precision square roots and divisions -- and every candidate thread then evaluates the test in three flops.
struct CertConsts { double a, b, tslack, lhs_scale; int square; int ok; };
__device__ __forceinline__ CertConsts cert_consts(const RerankParams& p, uint32_t q, double qn) {
    CertConsts c{0.0, 1.0, 0.0, 1.0, 0, 1};
    const double eps = (double)p.eps_coef;
    const double ndmax = sqrt((double)__uint_as_float(p.nd2max_bits[0]));
    const double fl = cert_floor(p);
    if (!(qn >= CERT_TINY_NORM)) { c.ok = 0; return c; }
    if (p.metric == COSINE) {
        const uint32_t mb = p.nd2max_bits[5];
        if (mb && !(__uint_as_float(~mb) >= (float)(CERT_TINY_NORM * CERT_TINY_NORM))) { c.ok = 0; return c; }
    }
    if (p.metric == EUCLID) { c.square = 1; c.lhs_scale = 1.0 + eps; }
    if (p.qerr && p.lb_scores) {
        // bf16 screening tier, Dot / Euclid: T is a LOWER-BOUND score (FusedBf16Params::margin) -- the bf16 rounding of
        // row and query, the MFMA accumulation and the row's share of the f32-fold budget were subtracted per row in the
        // kernel, so only the query's own terms are left here and no per-index maximum enters: one huge-norm row
        // loosens nobody's certificate but its own.  tslack: the f32 rounding of the margin fma.
        //   Dot:     e_k < Tl - fl                                   Euclid:  e_k^2 (1 + eps) < Tl + |q|^2 (1 - eps) - 4 fl
        c.tslack = 2.4e-7;
        c.a = p.metric == DOT ? -fl : qn * qn * (1.0 - eps) - 4.0 * fl;
        return c;
    }
    double E = 0.0, Ec = 0.0;
    if (p.qerr) {
        // bf16 screening tier (Cosine: the relative rounding error of a row is bounded by 2^-9 whatever its norm, so the
        // per-index maximum of it is a local quantity already; Dot / Euclid land here only for the raw-score diagnostics).
        // With e_q = q - bf16(q) (known) and e_d = d - bf16(d):
        //   dot(q,d) - dot(bf16 q, bf16 d) = e_q.d + bf16(q).e_d ,  |.| <= |e_q||d| + |bf16 q||e_d|   (Cauchy-Schwarz)
        // plus the f32 accumulation inside the MFMAs (c_acc |q||d|).  |bf16 q| <= 1.004 |q|; 1 % covers the f32
        // evaluation of the norms.  eps is the f32 tier's coefficient (oracle fold + fma chain).
        const double eq = (double)p.qerr[q];
        const double emax = sqrt((double)__uint_as_float(p.nd2max_bits[2]));
        const double rmax = sqrt((double)__uint_as_float(p.nd2max_bits[3]));
        const double cacc = (double)p.c_acc;
        E = 1.01 * (eq * ndmax + 1.004 * qn * emax) + cacc * qn * ndmax;
        Ec = 1.01 * (eq / qn + 1.004 * rmax) + cacc;
    }
    //   Dot:     e_k < T - E - eps |q| max|d| - fl
    //   Cosine:  e_k < 1 + T / |q| - Ec - eps - fl / (|q| 2^-40)
    //   Euclid:  e_k^2 (1 + eps) < T + |q|^2 - 2 E - eps (|q| + max|d|)^2 - 4 fl
    if (p.metric == DOT) c.a = -E - eps * qn * ndmax - fl;
    else if (p.metric == COSINE) { c.a = 1.0 - Ec - eps - fl / (qn * CERT_TINY_NORM); c.b = 1.0 / qn; }
    else { const double s = qn + ndmax; c.a = qn * qn - 2.0 * E - eps * s * s - 4.0 * fl; }
    return c;
}
__device__ __forceinline__ bool cert_eval(const CertConsts& c, float T, double ek) {
    if (!c.ok) return false;
    const double Tl = (double)T - fabs((double)T) * c.tslack;
    const double lhs = c.square ? ek * ek * c.lhs_scale : ek;
    return lhs < c.a + c.b * Tl;
}
__device__ __forceinline__ bool cert_test(const RerankParams& p, uint32_t q, float T, double ek, double qn) {
    return cert_eval(cert_consts(p, q, qn), T, ek);
}

// The inverse of cert_test: the smallest score T* such that cert_test(T) holds for every T > T*.  Every row whose
// ranking score exceeds it is PROVEN to lie beyond the k-th exact distance ek, so a filter pass with T* (rounded up) as
// its threshold keeps every row that can still matter (the "re-threshold" pass of vdb_flat.cpp).
__device__ __forceinline__ float score_cut(const RerankParams& p, uint32_t q, double ek, double qn) {
    const double eps = (double)p.eps_coef;
    const double ndmax = sqrt((double)__uint_as_float(p.nd2max_bits[0]));
    double E = 0.0, Ec = 0.0;
    if (p.qerr) {
        const double eq = (double)p.qerr[q];
        const double emax = sqrt((double)__uint_as_float(p.nd2max_bits[2]));
        const double rmax = sqrt((double)__uint_as_float(p.nd2max_bits[3]));
        const double cacc = (double)p.c_acc;
        E = 1.01 * (eq * ndmax + 1.004 * qn * emax) + cacc * qn * ndmax;
        Ec = 1.01 * (eq / qn + 1.004 * rmax) + cacc;
    }
    const double fl = cert_floor(p);
    if (!(qn >= CERT_TINY_NORM)) return __uint_as_float(0x7fc00000u);          // not certifiable on an MFMA tier: no cut
    if (p.metric == COSINE) {
        const uint32_t mb = p.nd2max_bits[5];
        if (mb && !(__uint_as_float(~mb) >= (float)(CERT_TINY_NORM * CERT_TINY_NORM))) return __uint_as_float(0x7fc00000u);
    }
    double t;
    if (p.qerr && p.lb_scores) {
        t = p.metric == DOT ? ek + fl : ek * ek - qn * qn + eps * (qn * qn + ek * ek) + 4.0 * fl;
        t += fabs(t) * 2.4e-7;
    }
    else if (p.metric == DOT) t = ek + E + eps * qn * ndmax + fl;
    else if (p.metric == COSINE) t = (ek - 1.0 + Ec + eps + fl / (qn * CERT_TINY_NORM)) * qn;
    else { const double s = qn + ndmax; t = ek * ek - qn * qn + 2.0 * E + eps * (s * s + ek * ek) + 4.0 * fl; }
    t += fabs(t) * 1e-6 + 1e-30;                                // slack: looser is safe
    float f = (float)t;
    if ((double)f < t) f = __uint_as_float(__float_as_uint(f) + (f >= 0.0f ? 1u : (uint32_t)-1));   // round towards +inf
    return f;
}

}  // namespace vdb

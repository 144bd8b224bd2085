// kernels_exact.h -- the device functions that more than one translation unit of kernels needs: the reference's exact-order
// arithmetic (src/distance.rs:37-73, src/vector.rs:35-37) and the screening tier's certificate with its inverse, the score
// cut.  Every includer is built with -ffp-contract=off: each multiply and add below rounds on its own.
#pragma once
#include "kernels.h"
#include "row_split.h"

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
// The same two folds over a slice of a row of the SPLIT layout (row_split.h) as the re-rank kernels stage it: xs holds the 16-bit
// hi words of the slice's n8 elements (n8 a multiple of 8: whole 16-byte pieces) and behind them their lo words.  Each f32 is
// rebuilt from its two halves, two elements per 32-bit word pair, and folded exactly as above: the same values in the same
// order, so the sums are those of the F32 layout bit for bit.
__device__ __forceinline__ void split_join16(const uint32_t* __restrict__ hi, const uint32_t* __restrict__ lo, float4 (&b)[4]) {
    uint4 h[2], l[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) { h[u] = *reinterpret_cast<const uint4*>(hi + 4 * u); l[u] = *reinterpret_cast<const uint4*>(lo + 4 * u); }
    const uint32_t hw[8] = {h[0].x, h[0].y, h[0].z, h[0].w, h[1].x, h[1].y, h[1].z, h[1].w};
    const uint32_t lw[8] = {l[0].x, l[0].y, l[0].z, l[0].w, l[1].x, l[1].y, l[1].z, l[1].w};
    uint32_t e[16];
#pragma unroll
    for (int u = 0; u < 8; ++u) split_join2(hw[u], lw[u], &e[2 * u], &e[2 * u + 1]);
#pragma unroll
    for (int u = 0; u < 4; ++u)
        b[u] = float4{__uint_as_float(e[4 * u]), __uint_as_float(e[4 * u + 1]), __uint_as_float(e[4 * u + 2]), __uint_as_float(e[4 * u + 3])};
}
__device__ __forceinline__ float split_elem(const float* xs, uint32_t n8, uint32_t i) {
    const uint16_t* w = reinterpret_cast<const uint16_t*>(xs);
    return __uint_as_float(split_join(w[i], w[n8 + i]));
}
__device__ __forceinline__ float fold_dot_part_split(const float* __restrict__ q, const float* __restrict__ xs, uint32_t n8, uint32_t d, float s) {
    const uint32_t* hi = reinterpret_cast<const uint32_t*>(xs);
    const uint32_t* lo = hi + n8 / 2;
    uint32_t i = 0;
    for (; i + 16 <= d; i += 16) {
        float4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = *reinterpret_cast<const float4*>(q + i + 4 * u);
        split_join16(hi + i / 2, lo + i / 2, b);
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
    for (; i < d; ++i) s = __fadd_rn(s, __fmul_rn(q[i], split_elem(xs, n8, i)));
    return s;
}
__device__ __forceinline__ float fold_sqdiff_part_split(const float* __restrict__ q, const float* __restrict__ xs, uint32_t n8, uint32_t d, float s) {
    const uint32_t* hi = reinterpret_cast<const uint32_t*>(xs);
    const uint32_t* lo = hi + n8 / 2;
    uint32_t i = 0;
    for (; i + 16 <= d; i += 16) {
        float4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = *reinterpret_cast<const float4*>(q + i + 4 * u);
        split_join16(hi + i / 2, lo + i / 2, b);
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
    for (; i < d; ++i) { float t = __fsub_rn(q[i], split_elem(xs, n8, i)); s = __fadd_rn(s, __fmul_rn(t, t)); }
    return s;
}
// A K slice [k0, k0 + wlen) of candidate row `row` into LDS at dst, by the 64 lanes of a wave, piece b of 64 x 16 bytes
// (global_load_lds: lane L lands at dst + 256 b floats + 16 L bytes).  F32: the wlen floats (wlen a multiple of 4).  SPLIT
// (ld % 64 == 0): the slice's hi piece, then its lo piece, each rounded up to whole 16 bytes -- n8 = (wlen + 7) & ~7 elements,
// the same byte count; the fold is then fold_*_part_split(.., n8, ..).  k0 is a multiple of 16 in both.
typedef __attribute__((address_space(3))) void* rr_lds_t;
typedef const __attribute__((address_space(1))) void* rr_glb_t;
__device__ __forceinline__ uint32_t slice_pieces(uint32_t wlen, bool split) {
    const uint32_t vpr = split ? ((wlen + 7u) & ~7u) / 4 : wlen / 4;
    return (vpr + 63) / 64;
}
__device__ __forceinline__ void stage_slice_piece(const float* __restrict__ rows, uint32_t ld, uint32_t row, uint32_t k0, uint32_t wlen, bool split,
                                                  uint32_t b, uint32_t lane, float* dst) {
    const uint32_t c4 = b * 64 + lane;
    if (!split) {
        if (c4 < wlen / 4)
            __builtin_amdgcn_global_load_lds((rr_glb_t)(rows + (size_t)row * ld + k0 + 4 * c4), (rr_lds_t)(dst + 256 * b), 16, 0, 0);
        return;
    }
    const uint32_t nch = ((wlen + 7u) & ~7u) / 8;                       // 16-byte pieces of each half
    if (c4 < 2 * nch) {
        const char* base = reinterpret_cast<const char*>(rows + (size_t)row * ld);
        const char* src = c4 < nch ? base + 2 * (size_t)k0 + 16 * c4 : base + 2 * (size_t)ld + 2 * (size_t)k0 + 16 * (c4 - nch);
        __builtin_amdgcn_global_load_lds((rr_glb_t)src, (rr_lds_t)(dst + 256 * b), 16, 0, 0);
    }
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
    if (metric == EUCLID) return distance_from_fold(EUCLID, fold_sqdiff(q, x, d), qn, xn);
    return distance_from_fold(metric, fold_dot(q, x, d), qn, xn);
}

// The same folds for ONE row against up to NQ queries at once (the bounded scans of the searches, the row scan of the HNSW
// build): one thread per row, the row read once, 16 floats at a time, and folded against every query in the reference's order --
// NQ independent chains.  Query j is the row qbase + qidx[j] * pitch; qidx is an array INSIDE the kernel's parameter struct and
// nq is wave-uniform, so every query address is a uniform expression of kernel parameters and the query elements come through
// scalar loads.  s[j] ends as fold_sqdiff / fold_dot of (query j, x); s[j] for j >= nq stays 0.
// (NIDX is the length of the index array, deduced: scan_rows_kernel<4> and <8> pass the 16-entry qrow of their parameter struct.)
template <int NQ, int NIDX>
__device__ __forceinline__ void fold_multi(int metric, const float* x, uint32_t d, const float* qbase, uint32_t pitch,
                                           const uint32_t (&qidx)[NIDX], uint32_t nq, float (&s)[NQ]) {
    static_assert(NQ <= NIDX, "one index per query");
    // The sums are folded in a local array and copied to s at the end.  Folding into s directly compiled, in every includer, to
    // a different block layout of the j < nq guards with 6 to 10 more VGPRs than the loop written out in the kernel had
    // (bounded_scan_kernel 32 -> 40, scan_rows_kernel<4> 28 -> 34, <8> 30 -> 40): the body is optimised before it is inlined, and
    // until then s is memory that x and qbase may alias.  With the local array the arithmetic and load counts and the VGPRs are
    // the written-out loop's (32, 30, 32, 52).
    float acc[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) acc[j] = 0.0f;
    uint32_t i = 0;
    for (; i + 16 <= d; i += 16) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(x + i + 4 * u);
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            if (j < (int)nq) {                                              // wave-uniform
                const float* q = qbase + (size_t)qidx[j] * pitch + i;       // uniform address: scalar loads
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 a = *reinterpret_cast<const float4*>(q + 4 * u);
                    if (metric == EUCLID) {
                        float t;
                        t = __fsub_rn(a.x, v[u].x); acc[j] = __fadd_rn(acc[j], __fmul_rn(t, t));
                        t = __fsub_rn(a.y, v[u].y); acc[j] = __fadd_rn(acc[j], __fmul_rn(t, t));
                        t = __fsub_rn(a.z, v[u].z); acc[j] = __fadd_rn(acc[j], __fmul_rn(t, t));
                        t = __fsub_rn(a.w, v[u].w); acc[j] = __fadd_rn(acc[j], __fmul_rn(t, t));
                    } else {
                        acc[j] = __fadd_rn(acc[j], __fmul_rn(a.x, v[u].x));
                        acc[j] = __fadd_rn(acc[j], __fmul_rn(a.y, v[u].y));
                        acc[j] = __fadd_rn(acc[j], __fmul_rn(a.z, v[u].z));
                        acc[j] = __fadd_rn(acc[j], __fmul_rn(a.w, v[u].w));
                    }
                }
            }
        }
    }
    for (; i < d; ++i) {
        const float xv = x[i];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            if (j < (int)nq) {
                const float a = qbase[(size_t)qidx[j] * pitch + i];
                if (metric == EUCLID) { float t = __fsub_rn(a, xv); acc[j] = __fadd_rn(acc[j], __fmul_rn(t, t)); }
                else acc[j] = __fadd_rn(acc[j], __fmul_rn(a, xv));
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NQ; ++j) s[j] = acc[j];
}

// ---------------------------------------------------------------------------------------------
// What the exhaustive re-ranks share (rerank_all_kernel, rerank_large_body, range_rerank_kernel): the LDS plan of a staged row,
// the staging of a chunk of candidate rows with their exact distances, and the sort of (ordered distance, id) pairs.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t NO_ROW = 0xffffffffu;                          // sRowIdx entry of a key that is skipped

// floats between two rows staged in LDS: the padded dimension, plus 4 where it is a multiple of 8 (bank spread of the float4 reads)
__host__ __device__ inline uint32_t rerank_row_stride(uint32_t dim) {
    const uint32_t dimp = (dim + 3) & ~3u;
    return dimp + ((dimp % 8 == 0) ? 4 : 0);
}

// One chunk of a candidate list, by a workgroup of THREADS threads (nthis <= THREADS keys at keys[0 .. nthis)): thread t < nthis
// reads key t, raises *sNanKey for a NaN-score key (score word 0) and puts the key's row into sRowIdx[t] -- NO_ROW if the row is
// at or beyond n_rows or masked out, BEFORE any address is formed from it; the waves then stage the valid rows into
// sR[t * ldp ..] with global_load_lds, 16 bytes per lane; thread t gets exact_distance(sQ, its row).  Returns false for a
// thread without a key or with a skipped one (*dist, *row untouched).  Every thread of the workgroup must call it: it holds
// two barriers; the caller places the one that ends the chunk.
template <uint32_t THREADS>
__device__ __forceinline__ bool stage_chunk_distances(const uint64_t* __restrict__ keys, uint32_t nthis, const float* __restrict__ rows,
                                                      uint32_t ld, uint32_t dim, uint32_t n_rows, const uint32_t* __restrict__ rowmask,
                                                      const float* __restrict__ nd, int metric, float qn, const float* sQ, float* sR,
                                                      uint32_t ldp, uint32_t* sRowIdx, uint32_t* sNanKey, float* dist, uint32_t* row_out,
                                                      bool split = false) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t dimp = (dim + 3) & ~3u, bpr = slice_pieces(dimp, split);
    if (tid < nthis) {
        const uint64_t key = keys[tid];
        const uint32_t row = (uint32_t)key;
        if ((uint32_t)(key >> 32) == 0u) *sNanKey = 1u;
        const bool ok = row < n_rows && (rowmask ? ((rowmask[row >> 5] >> (row & 31)) & 1u) : true);
        sRowIdx[tid] = ok ? row : NO_ROW;
    }
    __syncthreads();
    for (uint32_t u = wv; u < nthis * bpr; u += THREADS / 64) {
        const uint32_t r = u / bpr, b = u % bpr;
        const uint32_t row = sRowIdx[r];
        if (row != NO_ROW) stage_slice_piece(rows, ld, row, 0, dimp, split, b, lane, sR + (size_t)r * ldp);
    }
    __syncthreads();
    if (tid >= nthis) return false;
    const uint32_t row = sRowIdx[tid];
    if (row == NO_ROW) return false;
    if (split) {                                                    // (SPLIT: the caller's ldp holds (dimp + 7) & ~7 floats)
        const float* xs = sR + (size_t)tid * ldp;
        const uint32_t n8 = (dimp + 7u) & ~7u;
        const float f = metric == EUCLID ? fold_sqdiff_part_split(sQ, xs, n8, dim, 0.0f) : fold_dot_part_split(sQ, xs, n8, dim, 0.0f);
        *dist = distance_from_fold(metric, f, qn, nd[row]);
    } else *dist = exact_distance(metric, sQ, sR + (size_t)tid * ldp, dim, qn, nd[row]);
    *row_out = row;
    return true;
}

// Bitonic sort of the pairs (sDist[i], sId[i]), i < P (a power of two >= 2, unused slots hold the maximum), ascending by
// (ordered distance, id), by a workgroup of THREADS threads.  Ends with a barrier.
template <uint32_t THREADS>
__device__ __forceinline__ void bitonic_sort_pairs(uint32_t* sDist, uint64_t* sId, uint32_t P, uint32_t tid) {
    for (uint32_t size = 2; size <= P; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = tid; t < P / 2; t += THREADS) {
                const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const uint32_t da = sDist[lo], db = sDist[hi];
                const uint64_t ia = sId[lo], ib = sId[hi];
                const bool gt = da > db || (da == db && ia > ib);
                if (gt == up) { sDist[lo] = db; sDist[hi] = da; sId[lo] = ib; sId[hi] = ia; }
            }
            __syncthreads();
        }
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

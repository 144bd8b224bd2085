// kernels_range.hip -- the kernels of the exact RANGE search (vdb_search.cpp range_search): every eligible row
// whose reference distance d satisfies d <= r, ascending by (distance, id).  No reference counterpart (flat_index.rs:52-65 only
// answers "the k nearest"); the distances are the reference's (kernels_exact.h), so the result is the prefix with d <= r of the
// oracle's full ranking, bit for bit.
//   range_cut_kernel      radius -> filter threshold of the bf16 screening pass: score_cut, the inverse of the certificate
//   range_rerank_kernel   the tail of the screened route: every key that passed the filter evaluated exactly, kept if d <= r, sorted
// The exact range scan and its emit are not here: they are the kNN fallback's kernels (kernels_aux.hip) -- bounded_scan_kernel<true>,
// the one pass over the rows with the radius as the bound, and emit_multi_kernel with the total.  range_rerank_kernel stages and
// sorts with the helpers of kernels_exact.h that rerank_all_kernel uses.
// gfx950 only.  Built with -ffp-contract=off like every translation unit that computes a reference distance.
#include "kernels.h"
#include "kernels_exact.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace vdb {

// ---------------------------------------------------------------------------------------------
// Radius -> score cut.  score_cut(ek) is the smallest score T* such that every row scoring above it is PROVEN to lie strictly
// beyond ek (cert_test holds for every T > T*).  With ek = r: a row with d <= r scores at or below the cut, so a filter pass
// with the cut as its inclusive threshold keeps every row of the answer.  One thread per query.
//   * Euclid / Cosine distances are never negative: r < 0 is the empty answer and never reaches score_cut (Euclid squares ek);
//     the threshold is -inf, nothing but a NaN score passes.
//   * no finite cut (r = +-inf, r >= 2 under Cosine -- every row --, a tiny query norm, a NaN from the constants): nocut[q] = 1,
//     the exact range scan answers the query; its threshold is -inf so that it costs the filter pass nothing.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void range_cut_kernel(RangeCutParams p) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= p.nq) return;
    const float r = p.radii[q];
    const float ninf = __uint_as_float(0xff800000u);
    float thr = ninf;
    uint32_t nocut = 0;
    if (p.cert.metric != DOT && r < 0.0f) {
        // empty answer
    } else if (!(r == r) || r == __uint_as_float(0x7f800000u) || r == ninf || (p.cert.metric == COSINE && r >= 2.0f)) {
        nocut = 1;
    } else {
        const float cut = score_cut(p.cert, q, (double)r, (double)p.cert.qnorm[q]);
        if (!(cut == cut) || cut == __uint_as_float(0x7f800000u) || cut == ninf) nocut = 1;
        else thr = cut;
    }
    p.thr[q] = thr;
    p.nocut[q] = nocut;
}
void launch_range_cut(const RangeCutParams& p, hipStream_t s) {
    if (!p.nq) return;
    hipLaunchKernelGGL(range_cut_kernel, dim3((p.nq + 255) / 256), dim3(256), 0, s, p);
}

// ---------------------------------------------------------------------------------------------
// The tail of the screened route, one workgroup per query.  EVERY key the select delivered (up to 2048, any order) is evaluated
// with exact_distance, rows staged through LDS chunk by chunk (stage_chunk_distances, shared with rerank_all_kernel); the keys
// with d <= r go to a sort area of 2048 (ordered distance, id) pairs, which one bitonic network orders (bitonic_sort_pairs).  The first min(total, max_results) are
// written, the rest of the query's output row is padded (id ~0, NaN distance).  complete[q] = 0 when a NaN-score key was in the
// list (as rerank_all_kernel: the exact range scan answers); a truncated list is flagged by the select (overflow).
// Everything that comes from device memory is treated as untrusted: the key count is clamped to the list's stride and the sort
// area, a row index is compared with n_rows before any address is formed, a sort slot is compared with the area before the store.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t RG_THREADS = 512, RG_AREA = 2048;
constexpr size_t RG_LDS_PLAN = 150 * 1024;                       // the plan of launch_rerank_all: sort area + row slices stay within it
constexpr size_t RG_STATIC = RG_AREA * 12 + RG_THREADS * 4 + 64; // sDist + sId + sRowIdx + flags

__global__ __launch_bounds__(RG_THREADS) void range_rerank_kernel(RangeRerankParams p) {
    extern __shared__ __attribute__((aligned(16))) float sRows[];
    __shared__ uint32_t sDist[RG_AREA];
    __shared__ uint64_t sId[RG_AREA];
    __shared__ uint32_t sRowIdx[RG_THREADS];
    __shared__ uint32_t sAnyNan, sNanKey, sKept;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    uint32_t cnt = p.cand_cnt[q] < p.cand_stride ? p.cand_cnt[q] : p.cand_stride;
    if (cnt > RG_AREA) cnt = RG_AREA;
    const uint64_t* cand = p.cand + (size_t)q * p.cand_stride;
    if (tid == 0) { sAnyNan = 0; sNanKey = 0; sKept = 0; }
    for (uint32_t i = tid; i < RG_AREA; i += RG_THREADS) { sDist[i] = 0xffffffffu; sId[i] = ~0ull; }
    const uint32_t dimp = (p.dim + 3) & ~3u;
    const uint32_t ldp = p.lds_row_stride;
    const uint32_t chunk = p.lds_chunk < RG_THREADS ? p.lds_chunk : RG_THREADS;
    float* sQ = sRows;
    float* sR = sRows + ldp;
    const float* gq = p.qp + (size_t)q * p.ld;
    for (uint32_t i = tid * 4; i < dimp; i += RG_THREADS * 4) *reinterpret_cast<float4*>(sQ + i) = *reinterpret_cast<const float4*>(gq + i);
    __syncthreads();
    const float qn_f = p.qnorm[q];
    const float r = p.radii[q];
    for (uint32_t c0 = 0; c0 < cnt; c0 += chunk) {
        const uint32_t nthis = (cnt - c0 < chunk) ? cnt - c0 : chunk;
        float dist;
        uint32_t row;
        if (stage_chunk_distances<RG_THREADS>(cand + c0, nthis, p.rows, p.ld, p.dim, p.n_rows, p.rowmask, p.nd, p.metric, qn_f, sQ, sR, ldp,
                                              sRowIdx, &sNanKey, &dist, &row)) {
            if (dist != dist) sAnyNan = 1u;
            else if (dist <= r) {
                const uint32_t slot = atomicAdd(&sKept, 1u);
                if (slot < RG_AREA) { sDist[slot] = f32_to_ordered(dist); sId[slot] = p.row_ids[row]; }
            }
        }
        __syncthreads();
    }
    const uint32_t total = sKept < RG_AREA ? sKept : RG_AREA;
    uint32_t n2 = 2;
    while (n2 < total) n2 <<= 1;                                   // (<= RG_AREA: total is clamped)
    bitonic_sort_pairs<RG_THREADS>(sDist, sId, n2, tid);
    const uint32_t nout = total < p.max_results ? total : p.max_results;
    for (uint32_t i = tid; i < p.max_results; i += RG_THREADS) {
        const size_t o = (size_t)q * p.max_results + i;
        if (i < nout) { p.out_ids[o] = sId[i]; p.out_dists[o] = ordered_to_f32(sDist[i]); }
        else { p.out_ids[o] = ~0ull; p.out_dists[o] = __uint_as_float(0x7fc00000u); }
    }
    if (tid == 0) {
        p.out_counts[q] = nout;
        if (p.out_totals) p.out_totals[q] = total;
        if (sAnyNan) atomicOr(p.status, ST_NAN);
        p.complete[q] = sNanKey ? 0u : 1u;
        p.n_keys[q] = cnt;
    }
}
void launch_range_rerank(const RangeRerankParams& p, uint32_t nq, hipStream_t s) {
    if (!nq) return;
    RangeRerankParams q = p;
    q.lds_row_stride = rerank_row_stride(p.dim);
    // rows of the slice area: what the plan leaves beside the sort area, at least the query row and one candidate row (dim <= 16384)
    const size_t row_bytes = (size_t)q.lds_row_stride * 4;
    size_t rows_fit = (RG_LDS_PLAN - RG_STATIC) / row_bytes;
    if (rows_fit < 2) rows_fit = 2;
    q.lds_chunk = (uint32_t)std::min<size_t>(RG_THREADS, rows_fit - 1);
    const size_t lds = (size_t)(q.lds_chunk + 1) * row_bytes;
    hipLaunchKernelGGL(range_rerank_kernel, dim3(nq), dim3(RG_THREADS), lds, s, q);
}

}  // namespace vdb

// kernels_recommend.hip -- the two device steps that turn "recommend from stored examples" (vdb_flat_recommend_batch, DESIGN.md
// 4.14) into the ordinary batched search: the query is a fold of rows the index already holds, and every example has to leave
// the result.
//   - fold_examples_kernel writes q_b into the dense query block [nq][dim] the search reads.  Per element j, in f32 and without
//     contraction (the library is built with -ffp-contract=off): sp = p_1[j], then sp = sp + p_i[j] for i = 2..np -- a LEFT fold in
//     list order that starts from the first row, not from 0 (-0.0 survives, np = 1 is the stored row itself); ap = sp for
//     np = 1, else sp * rp with rp = 1.0f / (float)np computed on the host (a multiply, never a device division); without
//     negatives q[j] = ap, otherwise an is built from the negatives in the same way and q[j] = ap + (ap - an).  Lanes run along
//     the row (16 bytes per lane when dim and ld are multiples of 4, as gather_rows_kernel); a workgroup covers FOLD_ELEMS
//     elements of one request, the grid covers nq x ceil(dim / FOLD_ELEMS).  The loads of the next four examples are issued
//     ahead of the adds; the ADDS happen in list order.  The row stride is ld, not dim: the padding is never read.  A row number
//     at or above n_rows (or a list the host could not have sent) makes the workgroup leave before it touches a row.
//   - strike_set_kernel removes every entry whose id is AMONG the request's example ids from its result list (k + m entries
//     were asked for) and closes the gaps in order; the list is cut to kcut.  One workgroup per request.  The example ids (at
//     most RECOMMEND_MAX_EXAMPLES) go into LDS; entries are compared by 64-bit id EQUALITY among the first count[b] entries only --
//     never by position or distance, and no id value is special (2^64 - 1 is an ordinary id).  The compaction runs in chunks of
//     one workgroup: every lane reads entry i, the kept lanes are ranked (wave64 ballot + popcount, cross-wave prefix in LDS),
//     the workgroup synchronises, every kept lane writes its entry at kept_so_far + rank <= i; a chunk only writes entries that
//     this or an earlier chunk has already read.  Nothing at or past count[b], or at or past kcut, is written.
// gfx950 only.
#include "kernels.h"

namespace vdb {

constexpr uint32_t REC_THREADS = 256, REC_WAVES = REC_THREADS / 64;
constexpr uint32_t FOLD_ELEMS = REC_THREADS * 4;                           // elements of a row per workgroup, both paths

__device__ __forceinline__ float fold_add(float a, float b) { return a + b; }
__device__ __forceinline__ float4 fold_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float fold_scale(float a, float r) { return a * r; }
__device__ __forceinline__ float4 fold_scale(float4 a, float r) { return make_float4(a.x * r, a.y * r, a.z * r, a.w * r); }
__device__ __forceinline__ float fold_away(float ap, float an) { return ap + (ap - an); }
__device__ __forceinline__ float4 fold_away(float4 ap, float4 an) {
    return make_float4(ap.x + (ap.x - an.x), ap.y + (ap.y - an.y), ap.z + (ap.z - an.z), ap.w + (ap.w - an.w));
}

// The average of rows row[0..n) at element offset `at` (in units of V), n >= 1: the loads of four rows ahead of their adds, the
// adds one after the other in list order.
template <typename V>
__device__ __forceinline__ V fold_side(const float* __restrict__ rows, uint32_t ld, const uint32_t* row, uint32_t n, uint32_t at, float r) {
    auto ld_row = [&](uint32_t i) { return reinterpret_cast<const V*>(rows + (size_t)row[i] * ld)[at]; };
    V acc = ld_row(0);
    uint32_t i = 1;
    for (; i + 4 <= n; i += 4) {
        const V a = ld_row(i), b = ld_row(i + 1), c = ld_row(i + 2), d = ld_row(i + 3);
        acc = fold_add(acc, a);
        acc = fold_add(acc, b);
        acc = fold_add(acc, c);
        acc = fold_add(acc, d);
    }
    for (; i < n; ++i) acc = fold_add(acc, ld_row(i));
    return n == 1 ? acc : fold_scale(acc, r);
}

template <typename V>
__device__ __forceinline__ V fold_query(const float* __restrict__ rows, uint32_t ld, const uint32_t* row, uint32_t np, uint32_t nn,
                                        uint32_t at, float rp, float rn) {
    const V ap = fold_side<V>(rows, ld, row, np, at, rp);
    if (nn == 0) return ap;
    return fold_away(ap, fold_side<V>(rows, ld, row + np, nn, at, rn));
}

__global__ __launch_bounds__(REC_THREADS) void fold_examples_kernel(const float* __restrict__ rows, uint32_t ld, uint32_t dim,
                                                                    uint32_t n_rows, RecommendLists L, uint32_t nq, uint32_t chunks,
                                                                    float* __restrict__ out) {
    __shared__ uint32_t sRow[RECOMMEND_MAX_EXAMPLES];
    __shared__ uint32_t sBad;
    const uint32_t b = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    if (b >= nq) return;
    const uint32_t o0 = L.offs[b], o1 = L.offs[b + 1], np = L.n_pos[b];
    if (o1 < o0 || o1 - o0 > RECOMMEND_MAX_EXAMPLES || np == 0 || np > o1 - o0) return;   // (the host refused such a list)
    const uint32_t m = o1 - o0;
    if (threadIdx.x == 0) sBad = 0;
    __syncthreads();
    if (threadIdx.x < m) {
        const uint32_t r = L.rows[o0 + threadIdx.x];
        sRow[threadIdx.x] = r;
        if (r >= n_rows) sBad = 1;
    }
    __syncthreads();
    if (sBad) return;                                                      // (the host resolved every row; never read outside the store)
    const float rp = L.recip[2 * (size_t)b], rn = L.recip[2 * (size_t)b + 1];
    float* dst = out + (size_t)b * dim;
    if (((dim | ld) & 3u) == 0) {
        const uint32_t i = chunk * REC_THREADS + threadIdx.x;              // in float4s
        if (i < dim / 4) reinterpret_cast<float4*>(dst)[i] = fold_query<float4>(rows, ld, sRow, np, m - np, i, rp, rn);
    } else {
        for (uint32_t t = 0; t < FOLD_ELEMS / REC_THREADS; ++t) {
            const uint32_t i = chunk * FOLD_ELEMS + t * REC_THREADS + threadIdx.x;
            if (i < dim) dst[i] = fold_query<float>(rows, ld, sRow, np, m - np, i, rp, rn);
        }
    }
}

void launch_fold_examples(const float* rows, uint32_t ld, uint32_t dim, uint32_t n_rows, const RecommendLists& L, uint32_t nq,
                          float* out, hipStream_t s) {
    if (nq == 0 || dim == 0) return;
    const uint32_t chunks = (dim + FOLD_ELEMS - 1) / FOLD_ELEMS;
    hipLaunchKernelGGL(fold_examples_kernel, dim3(nq * chunks), dim3(REC_THREADS), 0, s, rows, ld, dim, n_rows, L, nq, chunks, out);
}

__global__ __launch_bounds__(REC_THREADS) void strike_set_kernel(StrikeSetParams p) {
    __shared__ uint64_t sSet[RECOMMEND_MAX_EXAMPLES];
    __shared__ uint32_t sWave[REC_WAVES];
    const uint32_t b = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t* ids = p.ids + (size_t)b * p.kdev;
    float* dists = p.dists + (size_t)b * p.kdev;
    const uint32_t count = p.counts[b] < p.kdev ? p.counts[b] : p.kdev;
    const uint32_t o0 = p.offs[b], o1 = p.offs[b + 1];
    const uint32_t m = o1 - o0 < RECOMMEND_MAX_EXAMPLES ? o1 - o0 : RECOMMEND_MAX_EXAMPLES;   // (the host refused a longer list)
    if (threadIdx.x < m) sSet[threadIdx.x] = p.ex_ids[o0 + threadIdx.x];
    __syncthreads();
    uint32_t kept = 0, struck = 0;                                         // (kept: the same in every lane; struck: per wave)
    for (uint32_t base = 0; base < count && kept < p.kcut; base += REC_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const bool have = i < count;
        uint64_t id = 0;
        float d = 0.0f;
        if (have) { id = ids[i]; d = dists[i]; }
        bool keep = have;
        for (uint32_t e = 0; e < m; ++e) keep = keep && id != sSet[e];
        const unsigned long long kb = __ballot(keep);
        if (lane == 0) sWave[wave] = (uint32_t)__popcll(kb);
        __syncthreads();                                                   // every lane has read its entry; the wave totals are in
        uint32_t before = kept, total = 0;
        for (uint32_t w = 0; w < REC_WAVES; ++w) {
            if (w < wave) before += sWave[w];
            total += sWave[w];
        }
        const uint32_t pos = before + (uint32_t)__popcll(kb & ((1ull << lane) - 1ull));   // kept entries in front of this one
        if (keep && pos < p.kcut) { ids[pos] = id; dists[pos] = d; }       // (pos <= i: already read)
        // struck entries in front of the kcut-th kept one; those behind it belong to no answer
        struck += (uint32_t)__popcll(__ballot(have && !keep && pos < p.kcut));
        kept += total;
        __syncthreads();                                                   // sWave is rewritten by the next chunk
    }
    if (threadIdx.x == 0) p.counts[b] = kept < p.kcut ? kept : p.kcut;
    if (lane == 0 && struck) atomicAdd(p.stats, struck);                   // (each wave counted its own lanes)
}

void launch_strike_set(const StrikeSetParams& p, uint32_t nq, hipStream_t s) {
    if (nq == 0) return;
    hipLaunchKernelGGL(strike_set_kernel, dim3(nq), dim3(REC_THREADS), 0, s, p);
}

}  // namespace vdb

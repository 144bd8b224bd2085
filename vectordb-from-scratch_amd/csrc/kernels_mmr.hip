// kernels_mmr.hip -- the greedy selection of the diverse top-k (vdb_flat_search_batch_mmr, include/vdb_flat.h "DIVERSE TOP-K",
// DESIGN.md 4.15): maximal marginal relevance over the candidates a search at depth m has left in HBM.
//   One workgroup per query, count_b = min(k_b, c_b) dependent steps.  The candidate's distance d, its nearest pair distance so far
//   (near), its device row, its picked flag and -- under Cosine -- its norm live in LDS, MMR_MAX_CANDIDATES entries each.  Thread t
//   owns candidates t, t + T, ...  In step s every thread folds the rows of its unpicked candidates against the row of the LAST
//   pick -- the exact-order folds of kernels_exact.h, one pair per thread, the pick's row read through a wave-uniform address --
//   lowers near, forms score = lambda * d - mu * near (two multiplies and a subtraction, each rounded on its own: the file is
//   built with -ffp-contract=off) and keeps its smallest (score is NaN, score, position).  The waves reduce by shuffles, the
//   workgroup through LDS, thread 0 appends the pick.  Pairs are evaluated only when another pick follows, and only against picks:
//   sum_{t=1}^{count-1} (c - t) of them per query, never an m x m matrix.
//   The norms of Cosine are recomputed from the rows (fold_sq and the correctly rounded square root): one fold per candidate, and
//   nothing but the rows and the lists is read, so the kernel can run over any block of rows.
//   Every row number is checked against n_rows before an address is formed from it.
// gfx950 only.
#include "kernels_exact.h"

namespace vdb {

constexpr uint32_t MMR_THREADS = 256, MMR_WAVES = MMR_THREADS / 64;

// The selection key: flag 0 = a number, 1 = a NaN score, 2 = no candidate; then the score by IEEE <, then the position.
struct MmrKey { uint32_t flag; float score; uint32_t pos; };

__device__ __forceinline__ bool mmr_before(const MmrKey& a, const MmrKey& b) {
    if (a.flag != b.flag) return a.flag < b.flag;
    if (a.flag == 0) {
        if (a.score < b.score) return true;
        if (b.score < a.score) return false;                               // (-0 and +0 fall through: equal)
    }
    return a.pos < b.pos;
}

__global__ __launch_bounds__(MMR_THREADS) void mmr_select_kernel(MmrParams p) {
    __shared__ float sD[MMR_MAX_CANDIDATES], sNear[MMR_MAX_CANDIDATES], sNorm[MMR_MAX_CANDIDATES];
    __shared__ uint32_t sRow[MMR_MAX_CANDIDATES];
    __shared__ uint8_t sPicked[MMR_MAX_CANDIDATES];
    __shared__ uint32_t sWFlag[MMR_WAVES], sWPos[MMR_WAVES];
    __shared__ float sWScore[MMR_WAVES];
    __shared__ uint32_t sPick, sBad;
    const uint32_t b = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t stride = p.stride < MMR_MAX_CANDIDATES ? p.stride : MMR_MAX_CANDIDATES;
    const uint32_t c = p.counts[b] < stride ? p.counts[b] : stride;
    const uint32_t kq = p.ks[b] < p.kout ? p.ks[b] : p.kout;
    const uint32_t count = kq < c ? kq : c;
    const uint64_t* ids = p.ids + (size_t)b * p.stride;
    const float* dists = p.dists + (size_t)b * p.stride;
    const uint32_t* crow = p.cand_rows + (size_t)b * p.stride;
    uint64_t* out_ids = p.out_ids + (size_t)b * p.kout;
    float* out_dists = p.out_dists + (size_t)b * p.kout;
    float* out_scores = p.out_scores + (size_t)b * p.kout;
    const float lambda = p.lambda[b], mu = p.mu[b];
    if (tid == 0) sBad = 0;
    __syncthreads();
    for (uint32_t i = tid; i < c; i += MMR_THREADS) {
        const uint32_t r = crow[i];
        if (r >= p.n_rows) sBad = 1;
        sRow[i] = r;
        sD[i] = dists[i];
        sNear[i] = __builtin_inff();
        sPicked[i] = 0;
    }
    __syncthreads();
    if (sBad || count == 0) {                                              // (the host resolved every row; never read outside the store)
        if (tid == 0) {
            p.out_counts[b] = 0;
            if (sBad) atomicOr(p.status, 2u);
        }
        return;
    }
    if (p.metric == COSINE && count > 1)
        for (uint32_t i = tid; i < c; i += MMR_THREADS) sNorm[i] = __builtin_sqrtf(fold_sq(p.rows + (size_t)sRow[i] * p.ld, p.dim));
    if (tid == 0) {
        sPicked[0] = 1;
        sPick = 0;
        out_ids[0] = ids[0];
        out_dists[0] = sD[0];
        out_scores[0] = __fmul_rn(lambda, sD[0]);
        p.out_counts[b] = count;
    }
    __syncthreads();
    bool nan_pair = false;
    for (uint32_t t = 1; t < count; ++t) {
        const uint32_t last = (uint32_t)__builtin_amdgcn_readfirstlane((int)sPick);
        const float* prow = p.rows + (size_t)__builtin_amdgcn_readfirstlane((int)sRow[last]) * p.ld;   // wave-uniform
        const float pn = p.metric == COSINE ? sNorm[last] : 0.0f;
        MmrKey best{2u, 0.0f, 0xffffffffu};
        for (uint32_t i = tid; i < c; i += MMR_THREADS) {
            if (sPicked[i]) continue;
            const float D = exact_distance(p.metric, prow, p.rows + (size_t)sRow[i] * p.ld, p.dim, pn, p.metric == COSINE ? sNorm[i] : 0.0f);
            if (D != D) nan_pair = true;
            float near = sNear[i];
            near = (D != D || D < near) ? D : near;                        // a NaN pair is an error of the call; it sticks until then
            sNear[i] = near;
            const float score = __fsub_rn(__fmul_rn(lambda, sD[i]), __fmul_rn(mu, near));
            const MmrKey key{score != score ? 1u : 0u, score, i};
            if (mmr_before(key, best)) best = key;                         // (ascending i: a tie keeps the earlier position)
        }
#pragma unroll
        for (uint32_t o = 32; o > 0; o >>= 1) {
            const MmrKey other{(uint32_t)__shfl_xor((int)best.flag, (int)o), __shfl_xor(best.score, (int)o), (uint32_t)__shfl_xor((int)best.pos, (int)o)};
            if (mmr_before(other, best)) best = other;
        }
        if (lane == 0) { sWFlag[wave] = best.flag; sWScore[wave] = best.score; sWPos[wave] = best.pos; }
        __syncthreads();
        if (tid == 0) {
            MmrKey w{sWFlag[0], sWScore[0], sWPos[0]};
            for (uint32_t v = 1; v < MMR_WAVES; ++v) {
                const MmrKey o{sWFlag[v], sWScore[v], sWPos[v]};
                if (mmr_before(o, w)) w = o;
            }
            // (t < count <= c: an unpicked candidate exists, so w.pos < c)
            if (w.pos < c) {
                sPicked[w.pos] = 1;
                sPick = w.pos;
                out_ids[t] = ids[w.pos];
                out_dists[t] = sD[w.pos];
                out_scores[t] = w.score;
            }
        }
        __syncthreads();
    }
    if (__any(nan_pair) && lane == 0) atomicOr(p.status, 1u);
}

void launch_mmr_select(const MmrParams& p, uint32_t nq, hipStream_t s) {
    if (nq == 0) return;
    hipLaunchKernelGGL(mmr_select_kernel, dim3(nq), dim3(MMR_THREADS), 0, s, p);
}

}  // namespace vdb

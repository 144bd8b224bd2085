// kernels_distinct.hip -- the device steps of "one nearest row per group" (vdb_flat_search_batch_distinct): a
// ranked result list is collapsed by the group code a metadata column gives each id, and, where one group owns more of a list
// than a search can return, an id mask is written that leaves the groups already answered out of the next search.
//   - distinct_first_kernel walks one list of up to 1024 (id, distance) entries, ascending by (distance, id) as the search wrote
//     it.  Entry i is KEPT iff its code is -1 (no such field, or the id lies beyond the column: such a row is its own group) or
//     no entry j < i of the list has the same code.  The (code, position) pairs are sorted by the bitonic network the re-rank
//     kernels use and the first of every run of equal codes is marked: the lowest position of the run, that is the group's
//     nearest row.  An order-preserving prefix sum over the marks gives every kept entry its place; the first k are written --
//     id, the distance bits as they are, the code -- the rest of the answer row is padded (~0, NaN, -1), and the number kept and
//     the completeness flag follow.  complete = k rows are kept, or the list is shorter than the depth asked for (every eligible
//     row was seen).  APPEND mode starts behind the rows the answer already holds and does not look at them again: the list then
//     comes from a search under the mask of exclude_groups_kernel, which holds no row of a group already answered.
//   - exclude_groups_kernel writes that mask: the caller's mask (or all ones) over [0, bits), every id cleared whose code is
//     among the codes the answer holds.  The codes (at most 1024) are sorted in LDS and looked up by binary search.  A wave
//     takes 64 mask words: in step j lane l reads the code of id 64 (w0 + j) + l -- consecutive lanes, consecutive codes -- and
//     the ballot of "stays eligible" IS word w0 + j, which lane j keeps; after 64 steps every lane stores its one word.  Bits at
//     or beyond `bits` are clear.  exclude_ids_kernel then clears the kept rows that have NO group one by one with a vector
//     atomic AND: each is its own group and would otherwise be found again.
// Everything read from device memory is untrusted, as in kernels_range.hip: a count is clamped to its stride, an id is compared
// with the column's length before an address is formed, an output slot with its capacity before the store.  No id value is a
// flag: 2^32 - 1 is an ordinary id, ~0 only pads.  One workgroup per list; both kernels are short latency chains beside the
// searches they sit between.  gfx950 only.
#include "kernels.h"
#include "kernels_exact.h"

#include <algorithm>

namespace vdb {

constexpr uint32_t DG_THREADS = 256, DG_PER = DISTINCT_MAX_LIST / DG_THREADS;   // 4 consecutive list entries per thread in the scan
static_assert(DG_PER * DG_THREADS == DISTINCT_MAX_LIST, "the scan covers the list exactly");

__global__ __launch_bounds__(DG_THREADS) void distinct_first_kernel(DistinctFirstParams p) {
    __shared__ uint32_t sKey[DISTINCT_MAX_LIST];                           // the code as an unsigned sort key
    __shared__ uint64_t sPos[DISTINCT_MAX_LIST];                           // the entry's position in the list
    __shared__ int32_t sCode[DISTINCT_MAX_LIST];
    __shared__ uint32_t sKeep[DISTINCT_MAX_LIST];
    __shared__ uint32_t sScan[DG_THREADS];
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    const uint32_t b = p.dest ? p.dest[j] : j;
    if (b >= p.n_answers) return;                                          // (uniform: the whole workgroup leaves)
    const uint32_t stride = p.stride < DISTINCT_MAX_LIST ? p.stride : DISTINCT_MAX_LIST;
    const uint32_t count = p.counts[j] < stride ? p.counts[j] : stride;
    const uint64_t* ids = p.ids + (size_t)j * p.stride;
    const float* dists = p.dists + (size_t)j * p.stride;
    const uint32_t k = p.k < p.kstride ? p.k : p.kstride;
    uint32_t base = 0;
    if (p.append) base = p.kept[b] < k ? p.kept[b] : k;

    uint32_t P = 2;
    while (P < count) P <<= 1;                                             // (<= DISTINCT_MAX_LIST: count is clamped)
    for (uint32_t i = tid; i < DISTINCT_MAX_LIST; i += DG_THREADS) {
        int32_t code = -1;
        if (i < count) {
            const uint64_t id = ids[i];
            if (id < p.codes_len) code = p.codes[id];
        }
        sCode[i] = code;
        sKeep[i] = (i < count && code == -1) ? 1u : 0u;
        // a row without a group needs no run: it sorts behind every code together with the padding and is never marked below
        const bool grouped = i < count && code != -1;
        sKey[i] = grouped ? (uint32_t)code : 0xffffffffu;
        sPos[i] = grouped ? (uint64_t)i : ~0ull;
    }
    __syncthreads();
    bitonic_sort_pairs<DG_THREADS>(sKey, sPos, P, tid);
    for (uint32_t i = tid; i < P; i += DG_THREADS) {
        const uint64_t pos = sPos[i];
        if (pos < count && (i == 0 || sKey[i - 1] != sKey[i])) sKeep[(uint32_t)pos] = 1u;
    }
    __syncthreads();

    // order-preserving compaction: each thread owns DG_PER consecutive entries; an inclusive scan of the per-thread sums
    uint32_t mine = 0;
    for (uint32_t e = 0; e < DG_PER; ++e) mine += sKeep[tid * DG_PER + e];
    sScan[tid] = mine;
    __syncthreads();
    for (uint32_t off = 1; off < DG_THREADS; off <<= 1) {
        const uint32_t add = tid >= off ? sScan[tid - off] : 0u;
        __syncthreads();
        sScan[tid] += add;
        __syncthreads();
    }
    const uint32_t total_new = sScan[DG_THREADS - 1];
    uint32_t slot = base + sScan[tid] - mine;
    uint64_t* oi = p.out_ids + (size_t)b * p.kstride;
    float* od = p.out_dists + (size_t)b * p.kstride;
    int32_t* oc = p.out_codes + (size_t)b * p.kstride;
    for (uint32_t e = 0; e < DG_PER; ++e) {
        const uint32_t i = tid * DG_PER + e;
        if (!sKeep[i]) continue;
        if (slot < k) { oi[slot] = ids[i]; od[slot] = dists[i]; oc[slot] = sCode[i]; }
        ++slot;
    }
    const uint64_t total = (uint64_t)base + total_new;
    const uint32_t kept = total < k ? (uint32_t)total : k;
    for (uint32_t i = kept + tid; i < p.kstride; i += DG_THREADS) {
        oi[i] = ~0ull; od[i] = __uint_as_float(0x7fc00000u); oc[i] = -1;
    }
    if (tid == 0) {
        p.kept[b] = kept;
        p.complete[b] = (total >= p.k || p.counts[j] < p.depth || p.exhaustive) ? 1u : 0u;
    }
}

void launch_distinct_first(const DistinctFirstParams& p, uint32_t n_lists, hipStream_t s) {
    if (n_lists == 0) return;
    hipLaunchKernelGGL(distinct_first_kernel, dim3(n_lists), dim3(DG_THREADS), 0, s, p);
}

// ascending bitonic sort of P (a power of two >= 2) keys in LDS by a workgroup of DG_THREADS; ends with a barrier
__device__ __forceinline__ void bitonic_sort_keys(uint32_t* sK, uint32_t P, uint32_t tid) {
    for (uint32_t size = 2; size <= P; size <<= 1)
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = tid; t < P / 2; t += DG_THREADS) {
                const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const uint32_t a = sK[lo], c = sK[hi];
                if ((a > c) == up) { sK[lo] = c; sK[hi] = a; }
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(DG_THREADS) void exclude_groups_kernel(ExcludeGroupsParams p) {
    __shared__ uint32_t sEx[DISTINCT_MAX_LIST];                            // the codes to leave out, ascending; 0xffffffff (= -1, never excluded) pads
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t kstride = p.kstride < DISTINCT_MAX_LIST ? p.kstride : DISTINCT_MAX_LIST;
    const uint32_t n_kept = p.kept[p.answer] < kstride ? p.kept[p.answer] : kstride;
    const int32_t* kc = p.out_codes + (size_t)p.answer * p.kstride;
    uint32_t P = 2;
    while (P < n_kept) P <<= 1;
    for (uint32_t i = tid; i < P; i += DG_THREADS) sEx[i] = i < n_kept ? (uint32_t)kc[i] : 0xffffffffu;
    __syncthreads();
    bitonic_sort_keys(sEx, P, tid);
    const uint64_t words = (p.bits + 63) >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * (DG_THREADS / 64) + (tid >> 6), n_waves = (uint64_t)gridDim.x * (DG_THREADS / 64);
    for (uint64_t w0 = wave * 64; w0 < words; w0 += n_waves * 64) {       // (w0 and the trip count are the same in every lane of a wave)
        const uint64_t mine_w = w0 + lane;
        const uint64_t src = mine_w < words ? (p.src ? p.src[mine_w] : ~0ull) : 0ull;
        uint64_t out = 0;
        for (uint32_t step = 0; step < 64; ++step) {
            const uint64_t sw = __shfl((unsigned long long)src, (int)step);                    // word w0 + step of the source mask, wave-uniform
            if (sw == 0) continue;                                         // (nothing eligible here: no code is read)
            const uint64_t id = ((w0 + step) << 6) + lane;
            bool ok = id < p.bits && ((sw >> lane) & 1ull);
            if (ok && id < p.codes_len) {
                const uint32_t code = (uint32_t)p.codes[id];
                if (code != 0xffffffffu) {
                    uint32_t lo = 0, hi = P;                               // lower bound of code in sEx[0, P)
                    while (lo < hi) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (sEx[mid] < code) lo = mid + 1; else hi = mid;
                    }
                    if (lo < P && sEx[lo] == code) ok = false;
                }
            }
            const uint64_t word = __ballot(ok);
            if (lane == step) out = word;
        }
        if (mine_w < words) p.mask[mine_w] = out;
    }
}

__global__ __launch_bounds__(DG_THREADS) void exclude_ids_kernel(ExcludeGroupsParams p) {
    const uint32_t kstride = p.kstride < DISTINCT_MAX_LIST ? p.kstride : DISTINCT_MAX_LIST;
    const uint32_t n_kept = p.kept[p.answer] < kstride ? p.kept[p.answer] : kstride;
    for (uint32_t i = threadIdx.x; i < n_kept; i += DG_THREADS) {
        if (p.out_codes[(size_t)p.answer * p.kstride + i] != -1) continue;
        const uint64_t id = p.out_ids[(size_t)p.answer * p.kstride + i];
        if (id < p.bits) atomicAnd(reinterpret_cast<unsigned long long*>(p.mask + (id >> 6)), ~(1ull << (id & 63)));
    }
}

void launch_exclude_groups(const ExcludeGroupsParams& p, uint32_t n_cu, hipStream_t s) {
    const uint64_t words = (p.bits + 63) >> 6;
    if (words == 0) return;
    const uint64_t per_block = (uint64_t)(DG_THREADS / 64) * 64;           // mask words one workgroup writes per trip
    const uint64_t want = (words + per_block - 1) / per_block;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(want, (uint64_t)std::max<uint32_t>(n_cu, 1) * 4);
    hipLaunchKernelGGL(exclude_groups_kernel, dim3(grid), dim3(DG_THREADS), 0, s, p);
    hipLaunchKernelGGL(exclude_ids_kernel, dim3(1), dim3(DG_THREADS), 0, s, p);
}

}  // namespace vdb

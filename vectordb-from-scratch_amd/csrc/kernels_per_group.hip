// kernels_per_group.hip -- the device steps of "the k nearest groups with up to g rows of each" (vdb_flat_search_batch_per_group,
// DESIGN.md 4.16).  The groups are the answers of the search by group (kernels_distinct.hip); the kernels here list the rows of
// the wanted groups and rank only those.
//   - per_group_list_kernel streams over the device rows, one thread per row: the id, the live bit, the id-mask bit and codes[id].
//     A row that is live, admitted by the mask, has id < the column's length and a code found in the table of wanted codes
//     (ascending, distinct, >= 0; binary search, in LDS when it fits) belongs to that code's member list.  COUNT mode adds it to
//     the code's counter; SCATTER mode -- after the host has turned the counts into offsets -- takes a place from the code's
//     cursor and writes the row there as a candidate key.  The order inside a list is whatever the atomics give; no result
//     depends on it.  A code the host gave length 0 (a giant, see below) is counted and not listed.
//   - per_group_init_kernel writes the answer every (query, group) pair starts with: the representative as its single member.
//   - per_group_fill_kernel, one workgroup per (query, group) pair: the pair's list is walked in chunks, each chunk's rows staged
//     into LDS and evaluated with exact_distance (stage_chunk_distances, as the exhaustive re-ranks do), the best g by (ordered
//     distance, id) kept across chunks with the pair sort; members and size are written, a NaN distance raises the status word,
//     and member 0 is compared with the representative (id and distance bits): a difference is counted.
//   - per_group_code_mask_kernel writes the mask "caller's mask AND code == c" for a group whose list is beyond the fill's
//     capacity (a giant): its queries are searched the ordinary way under it, and per_group_place_kernel puts their lists into
//     the pairs' places, with the same comparison of member 0.
// Everything read from device memory is untrusted, as in kernels_distinct.hip: a count is clamped to its capacity, an id is
// compared with the column's length and a row with n_rows before an address is formed, an output slot with its capacity before
// the store.  No id value is a flag.  Built with -ffp-contract=off like every translation unit that computes a reference
// distance.  gfx950 only.
#include "kernels.h"
#include "kernels_exact.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace vdb {

constexpr uint32_t PG_THREADS = 256;
constexpr uint32_t PG_LDS_CODES = 4096;                                    // wanted codes the list kernel keeps in LDS
constexpr uint32_t PG_AREA = 512;                                          // sort area: the best g <= 32 and a chunk of <= 256
static_assert(PER_GROUP_MAX_SIZE + PG_THREADS <= PG_AREA, "the best g and one chunk fit the sort area");

// the place of `code` in the ascending table tab[0, n), or n
__device__ __forceinline__ uint32_t wanted_place(const int32_t* tab, uint32_t n, int32_t code) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (tab[mid] < code) lo = mid + 1; else hi = mid;
    }
    return (lo < n && tab[lo] == code) ? lo : n;
}

template <bool SCATTER>
__global__ __launch_bounds__(PG_THREADS) void per_group_list_kernel(PerGroupListParams p) {
    __shared__ int32_t sTab[PG_LDS_CODES];
    const bool in_lds = p.n_wanted <= PG_LDS_CODES;
    if (in_lds) {
        for (uint32_t i = threadIdx.x; i < p.n_wanted; i += PG_THREADS) sTab[i] = p.wanted[i];
        __syncthreads();
    }
    const int32_t* tab = in_lds ? sTab : p.wanted;
    for (uint64_t r = (uint64_t)blockIdx.x * PG_THREADS + threadIdx.x; r < p.n_rows; r += (uint64_t)gridDim.x * PG_THREADS) {
        const uint32_t row = (uint32_t)r;
        if (p.live && !((p.live[row >> 5] >> (row & 31)) & 1u)) continue;
        const uint64_t id = p.row_ids[row];
        if (p.mask && !(id < p.mask_bits && ((p.mask[id >> 6] >> (id & 63)) & 1ull))) continue;
        if (id >= p.codes_len) continue;
        const int32_t code = p.codes[id];
        if (code < 0) continue;
        const uint32_t u = wanted_place(tab, p.n_wanted, code);
        if (u >= p.n_wanted) continue;
        if (!SCATTER) {
            atomicAdd(p.counts + u, 1u);
        } else {
            const uint32_t len = p.lens[u];
            if (len == 0) continue;
            const uint32_t pos = atomicAdd(p.cursor + u, 1u);
            const uint64_t at = (uint64_t)p.offs[u] + pos;
            if (pos < len && at < p.list_cap) p.list[at] = (1ull << 32) | row;     // a candidate key: score word not 0 (0 = a NaN score)
        }
    }
}

void launch_per_group_list(const PerGroupListParams& p, bool scatter, uint32_t n_cu, hipStream_t s) {
    if (!p.n_rows || !p.n_wanted) return;
    const uint64_t want = ((uint64_t)p.n_rows + PG_THREADS - 1) / PG_THREADS;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(want, (uint64_t)std::max<uint32_t>(n_cu, 1) * 8);
    if (scatter) hipLaunchKernelGGL(per_group_list_kernel<true>, dim3(grid), dim3(PG_THREADS), 0, s, p);
    else hipLaunchKernelGGL(per_group_list_kernel<false>, dim3(grid), dim3(PG_THREADS), 0, s, p);
}

__global__ __launch_bounds__(PG_THREADS) void per_group_init_kernel(PerGroupInitParams p) {
    const uint64_t slot = (uint64_t)blockIdx.x * PG_THREADS + threadIdx.x;
    if (slot >= (uint64_t)p.nq * p.kmax) return;
    const uint32_t b = (uint32_t)(slot / p.kmax), j = (uint32_t)(slot % p.kmax);
    const uint32_t kept = p.kept[b] < p.kmax ? p.kept[b] : p.kmax;
    const bool have = j < kept;
    uint64_t* oi = p.out_ids + slot * p.g;
    float* od = p.out_dists + slot * p.g;
    for (uint32_t m = 0; m < p.g; ++m) { oi[m] = ~0ull; od[m] = __uint_as_float(0x7fc00000u); }
    if (have) { oi[0] = p.rep_ids[slot]; od[0] = p.rep_dists[slot]; }
    p.out_sizes[slot] = have ? 1u : 0u;
}

void launch_per_group_init(const PerGroupInitParams& p, hipStream_t s) {
    const uint64_t n = (uint64_t)p.nq * p.kmax;
    if (!n || !p.g) return;
    hipLaunchKernelGGL(per_group_init_kernel, dim3((uint32_t)((n + PG_THREADS - 1) / PG_THREADS)), dim3(PG_THREADS), 0, s, p);
}

__global__ __launch_bounds__(PG_THREADS) void per_group_fill_kernel(PerGroupFillParams p) {
    extern __shared__ __attribute__((aligned(16))) float sRows[];
    __shared__ uint32_t sDist[PG_AREA];
    __shared__ uint64_t sId[PG_AREA];
    __shared__ uint32_t sRowIdx[PG_THREADS];
    __shared__ uint32_t sAnyNan, sNanKey, sValid;
    __shared__ float sQn;
    const uint32_t tid = threadIdx.x;
    const uint32_t slot = p.pairs[2 * (size_t)blockIdx.x], u = p.pairs[2 * (size_t)blockIdx.x + 1];
    if ((uint64_t)slot >= (uint64_t)p.nq * p.kmax || u >= p.n_wanted) return;   // (uniform: the whole workgroup leaves)
    const uint32_t b = slot / p.kmax;
    const uint32_t g = p.g < PER_GROUP_MAX_SIZE ? p.g : PER_GROUP_MAX_SIZE;
    const uint64_t off = p.offs[u] < p.list_cap ? p.offs[u] : p.list_cap;
    const uint64_t room = p.list_cap - off;
    const uint32_t len = p.lens[u] < room ? p.lens[u] : (uint32_t)room;
    const uint64_t* list = p.list + off;
    const uint32_t ldp = p.lds_row_stride;
    const uint32_t chunk = p.lds_chunk < PG_THREADS ? p.lds_chunk : PG_THREADS;
    uint32_t P = 2;
    while (P < g + chunk) P <<= 1;                                         // (<= PG_AREA)
    float* sQ = sRows;
    float* sR = sRows + ldp;
    const float* gq = p.q + (size_t)b * p.dim;
    if (tid == 0) { sAnyNan = 0; sNanKey = 0; sValid = 0; }
    for (uint32_t i = tid; i < PG_AREA; i += PG_THREADS) { sDist[i] = 0xffffffffu; sId[i] = ~0ull; }
    for (uint32_t i = tid; i < ldp; i += PG_THREADS) sQ[i] = i < p.dim ? gq[i] : 0.0f;
    __syncthreads();
    if (tid == 0) sQn = p.metric == COSINE ? __builtin_sqrtf(fold_sq(sQ, p.dim)) : 0.0f;
    __syncthreads();
    const float qn = sQn;
    for (uint32_t c0 = 0; c0 < len; c0 += chunk) {
        const uint32_t nthis = (len - c0 < chunk) ? len - c0 : chunk;
        float dist;
        uint32_t row;
        const bool have = stage_chunk_distances<PG_THREADS>(list + c0, nthis, p.rows, p.ld, p.dim, p.n_rows, nullptr, p.nd, p.metric, qn,
                                                            sQ, sR, ldp, sRowIdx, &sNanKey, &dist, &row);
        if (tid < nthis) {
            uint32_t od = 0xffffffffu;
            uint64_t id = ~0ull;
            if (have) {
                if (dist != dist) sAnyNan = 1u;
                od = f32_to_ordered(dist);
                id = p.row_ids[row];
                atomicAdd(&sValid, 1u);
            }
            sDist[g + tid] = od;
            sId[g + tid] = id;
        }
        __syncthreads();
        bitonic_sort_pairs<PG_THREADS>(sDist, sId, P, tid);
        for (uint32_t i = g + tid; i < P; i += PG_THREADS) { sDist[i] = 0xffffffffu; sId[i] = ~0ull; }   // keep the best g only
        __syncthreads();
    }
    const uint32_t size = sValid < g ? sValid : g;
    uint64_t* oi = p.out_ids + (size_t)slot * p.g;
    float* od = p.out_dists + (size_t)slot * p.g;
    for (uint32_t m = tid; m < p.g; m += PG_THREADS) {
        if (m < size) { oi[m] = sId[m]; od[m] = ordered_to_f32(sDist[m]); }
        else { oi[m] = ~0ull; od[m] = __uint_as_float(0x7fc00000u); }
    }
    if (tid == 0) {
        p.out_sizes[slot] = size;
        if (sAnyNan) atomicOr(p.status, ST_NAN);
        const bool same = size > 0 && sId[0] == p.rep_ids[slot] && __float_as_uint(ordered_to_f32(sDist[0])) == __float_as_uint(p.rep_dists[slot]);
        if (!same && !sAnyNan) atomicAdd(p.status + 1, 1u);
    }
}

void launch_per_group_fill(const PerGroupFillParams& p, uint32_t n_pairs, hipStream_t s) {
    if (!n_pairs) return;
    PerGroupFillParams q = p;
    q.lds_row_stride = rerank_row_stride(p.dim);
    // the LDS plan of launch_rerank_all: the query row and a chunk of candidate rows within 150 KB (dim <= 16384: one row fits)
    const size_t row_bytes = (size_t)q.lds_row_stride * 4;
    size_t rows_fit = (150 * 1024) / row_bytes;
    if (rows_fit < 2) rows_fit = 2;
    q.lds_chunk = (uint32_t)std::min<size_t>(PG_THREADS, rows_fit - 1);
    const size_t lds = (size_t)(q.lds_chunk + 1) * row_bytes;
    hipLaunchKernelGGL(per_group_fill_kernel, dim3(n_pairs), dim3(PG_THREADS), lds, s, q);
}

// A wave takes 64 mask words as exclude_groups_kernel does: in step j lane l reads the code of id 64 (w0 + j) + l -- consecutive
// lanes, consecutive codes -- and the ballot of "eligible and of this code" IS word w0 + j, which lane j keeps.
__global__ __launch_bounds__(PG_THREADS) void per_group_code_mask_kernel(PerGroupCodeMaskParams p) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t words = (p.bits + 63) >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * (PG_THREADS / 64) + (tid >> 6), n_waves = (uint64_t)gridDim.x * (PG_THREADS / 64);
    for (uint64_t w0 = wave * 64; w0 < words; w0 += n_waves * 64) {        // (w0 and the trip count are the same in every lane of a wave)
        const uint64_t mine_w = w0 + lane;
        const uint64_t src = mine_w < words ? (p.src ? p.src[mine_w] : ~0ull) : 0ull;
        uint64_t out = 0;
        for (uint32_t step = 0; step < 64; ++step) {
            const uint64_t sw = __shfl((unsigned long long)src, (int)step);                    // word w0 + step of the source mask, wave-uniform
            if (sw == 0) continue;
            const uint64_t id = ((w0 + step) << 6) + lane;
            const bool ok = id < p.bits && ((sw >> lane) & 1ull) && id < p.codes_len && p.codes[id] == p.code;
            const uint64_t word = __ballot(ok);
            if (lane == step) out = word;
        }
        if (mine_w < words) p.mask[mine_w] = out;
    }
}

void launch_per_group_code_mask(const PerGroupCodeMaskParams& p, uint32_t n_cu, hipStream_t s) {
    const uint64_t words = (p.bits + 63) >> 6;
    if (words == 0) return;
    const uint64_t per_block = (uint64_t)(PG_THREADS / 64) * 64;
    const uint64_t want = (words + per_block - 1) / per_block;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(want, (uint64_t)std::max<uint32_t>(n_cu, 1) * 4);
    hipLaunchKernelGGL(per_group_code_mask_kernel, dim3(grid), dim3(PG_THREADS), 0, s, p);
}

__global__ __launch_bounds__(64) void per_group_place_kernel(PerGroupPlaceParams p) {
    const uint32_t i = blockIdx.x, m = threadIdx.x;
    const uint32_t slot = p.dest[i];
    if ((uint64_t)slot >= (uint64_t)p.nq * p.kmax) return;
    uint32_t size = p.counts[i] < p.stride ? p.counts[i] : p.stride;
    if (size > p.g) size = p.g;
    const uint64_t* ids = p.ids + (size_t)i * p.stride;
    const float* dists = p.dists + (size_t)i * p.stride;
    if (m < p.g) {
        const size_t o = (size_t)slot * p.g + m;
        if (m < size) { p.out_ids[o] = ids[m]; p.out_dists[o] = dists[m]; }
        else { p.out_ids[o] = ~0ull; p.out_dists[o] = __uint_as_float(0x7fc00000u); }
    }
    if (m == 0) {
        p.out_sizes[slot] = size;
        const bool same = size > 0 && ids[0] == p.rep_ids[slot] && __float_as_uint(dists[0]) == __float_as_uint(p.rep_dists[slot]);
        if (!same) atomicAdd(p.status + 1, 1u);
    }
}

void launch_per_group_place(const PerGroupPlaceParams& p, uint32_t n_lists, hipStream_t s) {
    if (!n_lists) return;
    static_assert(PER_GROUP_MAX_SIZE <= 64, "one thread per member");
    hipLaunchKernelGGL(per_group_place_kernel, dim3(n_lists), dim3(64), 0, s, p);
}

}  // namespace vdb

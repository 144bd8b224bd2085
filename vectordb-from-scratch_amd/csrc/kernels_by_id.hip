// kernels_by_id.hip -- the two device steps that turn "search by stored id" (vdb_flat_search_batch_by_id) into
// the ordinary batched search: the queries are rows the index already holds, and the query's own row has to leave its result.
//   - gather_rows_kernel copies the stored rows named by row[] into the dense query block [nq][dim] the search reads.  One wave
//     per query; consecutive lanes read consecutive floats of the row (16 bytes per lane when dim is a multiple of 4: rows start
//     on a 128-byte boundary because ld is a multiple of 32, and the destination row then starts on a 16-byte one).  The row
//     stride is ld, not dim: the padding is not copied.
//   - strike_self_kernel removes the entry whose id EQUALS self_id[b] from query b's result list (k + 1 entries were asked for)
//     and closes the gap in order; when the id is not in the list, the list is cut to k.  One workgroup per query.  The entry is
//     found by comparing 64-bit ids among the first count[b] entries only -- never by position or distance, and no id value is
//     special (2^64 - 1 is an ordinary id).  Ids in one result list are distinct, so at most one lane finds it.  The shift runs in
//     chunks of one workgroup: every lane reads entry i + 1, the workgroup synchronises, every lane writes entry i; a chunk only
//     writes entries that earlier chunks have already read.  Nothing at or past count[b] is written.
// gfx950 only.
#include "kernels.h"

namespace vdb {

constexpr uint32_t BYID_THREADS = 256, BYID_WAVES = BYID_THREADS / 64;

__global__ __launch_bounds__(BYID_THREADS) void gather_rows_kernel(const float* __restrict__ rows, uint32_t ld, uint32_t dim,
                                                                   uint32_t n_rows, const uint32_t* __restrict__ row, uint32_t nq,
                                                                   float* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t b = (uint64_t)blockIdx.x * BYID_WAVES + wave;
    if (b >= nq) return;
    const uint32_t r = row[b];
    if (r >= n_rows) return;                                               // (the host resolved every row; never read outside the store)
    const float* src = rows + (size_t)r * ld;
    float* dst = out + (size_t)b * dim;
    if ((dim & 3u) == 0) {
        const float4* src4 = reinterpret_cast<const float4*>(src);
        float4* dst4 = reinterpret_cast<float4*>(dst);
        for (uint32_t i = lane; i < dim / 4; i += 64) dst4[i] = src4[i];
    } else {
        for (uint32_t i = lane; i < dim; i += 64) dst[i] = src[i];
    }
}

void launch_gather_rows(const float* rows, uint32_t ld, uint32_t dim, uint32_t n_rows, const uint32_t* row, uint32_t nq, float* out,
                        hipStream_t s) {
    if (nq == 0 || dim == 0) return;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((nq + BYID_WAVES - 1) / BYID_WAVES), dim3(BYID_THREADS), 0, s, rows, ld, dim, n_rows,
                       row, nq, out);
}

__global__ __launch_bounds__(BYID_THREADS) void strike_self_kernel(StrikeSelfParams p) {
    __shared__ uint32_t sPos;
    const uint32_t b = blockIdx.x;
    uint64_t* ids = p.ids + (size_t)b * p.kdev;
    float* dists = p.dists + (size_t)b * p.kdev;
    const uint32_t count = p.counts[b] < p.kdev ? p.counts[b] : p.kdev;
    const uint64_t self = p.self_id[b];
    if (threadIdx.x == 0) sPos = 0xffffffffu;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < count; i += BYID_THREADS)
        if (ids[i] == self) atomicMin(&sPos, i);
    __syncthreads();
    const uint32_t pos = sPos;
    if (pos == 0xffffffffu) {                                              // not in the list: the last of the k + 1 goes
        if (threadIdx.x == 0 && count > p.k) {
            p.counts[b] = p.k;
            atomicAdd(p.stats + 1, 1u);
        }
        return;
    }
    for (uint32_t base = pos; base + 1 < count; base += BYID_THREADS) {    // (pos and count are the same in every lane)
        const uint32_t i = base + threadIdx.x;
        const bool move = i + 1 < count;
        uint64_t id = 0;
        float d = 0.0f;
        if (move) { id = ids[i + 1]; d = dists[i + 1]; }
        __syncthreads();
        if (move) { ids[i] = id; dists[i] = d; }
    }
    if (threadIdx.x == 0) {
        p.counts[b] = count - 1;
        atomicAdd(p.stats, 1u);
    }
}

void launch_strike_self(const StrikeSelfParams& p, uint32_t nq, hipStream_t s) {
    if (nq == 0) return;
    hipLaunchKernelGGL(strike_self_kernel, dim3(nq), dim3(BYID_THREADS), 0, s, p);
}

}  // namespace vdb

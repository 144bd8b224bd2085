// kernels_spv_select.h -- the exact top-k select of the sparse-vector index (DESIGN.md 4.20 "Select"), shared by the inverted route
// (kernels_spv.hip) and the row-major route (kernels_spv_rows.hip).  Device code of a workgroup of SPV_THREADS threads: an LDS
// buffer s_keys[SPV_SELECT_CAP] of unique 64-bit keys, its fill *s_cnt and the threshold *s_thr a later offer must beat.  The
// caller keeps a workgroup-uniform upper bound of the fill and calls spv_prune before a round of offers that might not fit.
#pragma once
#include "kernels.h"
#include "kernels_spv.h"

namespace vdb {

// Sorts s_keys[0, n) ascending (unique keys), keeps the kq smallest; returns how many are kept.  Called by the whole workgroup.
__device__ inline uint32_t spv_prune(uint64_t* s_keys, uint32_t* s_cnt, uint64_t* s_thr, uint32_t kq) {
    const uint32_t tid = threadIdx.x;
    __syncthreads();                                   // every push of the rounds before is in the buffer
    const uint32_t n = *s_cnt;
    uint32_t P = 2;
    while (P < n) P <<= 1;
    for (uint32_t i = n + tid; i < P; i += SPV_THREADS) s_keys[i] = EMPTY_KEY;
    __syncthreads();
    for (uint32_t k2 = 2; k2 <= P; k2 <<= 1)
        for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < P; i += SPV_THREADS) {
                const uint32_t o = i ^ j;
                if (o > i) {
                    const uint64_t x = s_keys[i], y = s_keys[o];
                    if ((x > y) == ((i & k2) == 0)) { s_keys[i] = y; s_keys[o] = x; }
                }
            }
            __syncthreads();
        }
    const uint32_t keep = min(n, kq);
    if (tid == 0) {
        *s_cnt = keep;
        *s_thr = (kq && n >= kq) ? s_keys[kq - 1] : EMPTY_KEY;
    }
    __syncthreads();
    return keep;
}

// One offer: the key enters the buffer if it beats the threshold.  The caller's bound keeps the slot below SPV_SELECT_CAP.
__device__ inline void spv_offer(uint64_t* s_keys, uint32_t* s_cnt, const uint64_t* s_thr, uint64_t key) {
    if (key < *s_thr) s_keys[atomicAdd(s_cnt, 1u)] = key;
}

}  // namespace vdb

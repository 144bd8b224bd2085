// kernels_split.hip -- the two conversions of the row store between its layouts (row_split.h): F32 -> SPLIT and back, in
// place.  gfx950 (MI355X) only.
//
// A row is converted where it lies: workgroups stride over batches of whole rows (as many as fit into 64 KB of LDS), read
// every element of the batch, write its image in the other layout into LDS, and only behind the barrier copy the image over
// the batch.  So no byte of a row is written before the whole row has been read, and no two workgroups touch one row.  The
// forward pass also reports whether any element it saw has an all-ones exponent (inf, NaN): the caller then converts straight
// back, because the hi word of two NaN families reads as zero.  Zero rows stay zero in both directions, so only the uploaded
// rows are walked.
#include <algorithm>

#include "kernels.h"
#include "row_split.h"

namespace vdb {

namespace {

constexpr uint32_t SPLIT_THREADS = 1024;
constexpr uint32_t SPLIT_LDS_WORDS = 16384;                              // 64 KB: one row of the largest dimension, 21 rows of 768

template <bool FWD>
__global__ __launch_bounds__(SPLIT_THREADS) void row_split_kernel(uint32_t* __restrict__ rows, uint32_t ld, uint32_t n_rows, uint32_t batch,
                                                                  uint32_t* __restrict__ nonfinite) {
    extern __shared__ __attribute__((aligned(16))) uint32_t sImg[];
    const uint32_t q4 = ld >> 2, half = ld >> 1;                        // 4-element groups of a row; 32-bit words of its hi piece
    bool bad = false;
    for (uint32_t r0 = blockIdx.x * batch; r0 < n_rows; r0 += gridDim.x * batch) {
        const uint32_t nr = n_rows - r0 < batch ? n_rows - r0 : batch;
        uint32_t* g = rows + (size_t)r0 * ld;
        const uint32_t groups = nr * q4;
#pragma unroll 4
        for (uint32_t i = threadIdx.x; i < groups; i += SPLIT_THREADS) {
            const uint32_t r = i / q4, c = i - r * q4;                    // elements 4c .. 4c + 3 of row r0 + r
            const uint32_t* grow = g + (size_t)r * ld;
            uint32_t* srow = sImg + r * ld;
            if (FWD) {
                const uint4 v = *reinterpret_cast<const uint4*>(grow + 4 * c);
                bad = bad || split_nonfinite(v.x) || split_nonfinite(v.y) || split_nonfinite(v.z) || split_nonfinite(v.w);
                uint2 hi, lo;
                split_pack2(v.x, v.y, &hi.x, &lo.x);
                split_pack2(v.z, v.w, &hi.y, &lo.y);
                *reinterpret_cast<uint2*>(srow + 2 * c) = hi;
                *reinterpret_cast<uint2*>(srow + half + 2 * c) = lo;
            } else {
                const uint2 hi = *reinterpret_cast<const uint2*>(grow + 2 * c);
                const uint2 lo = *reinterpret_cast<const uint2*>(grow + half + 2 * c);
                uint4 v;
                split_join2(hi.x, lo.x, &v.x, &v.y);
                split_join2(hi.y, lo.y, &v.z, &v.w);
                *reinterpret_cast<uint4*>(srow + 4 * c) = v;
            }
        }
        __syncthreads();                                                  // every element of the batch has been read
        for (uint32_t i = threadIdx.x; i < groups; i += SPLIT_THREADS)
            reinterpret_cast<uint4*>(g)[i] = reinterpret_cast<const uint4*>(sImg)[i];
        __syncthreads();
    }
    if (FWD && bad) atomicOr(nonfinite, 1u);
}

}  // namespace

void launch_row_split(float* rows, uint32_t ld, uint32_t n_rows, bool forward, uint32_t* nonfinite, uint32_t n_cu, hipStream_t s) {
    if (!n_rows || !ld || ld > SPLIT_LDS_WORDS) return;
    const uint32_t batch = std::max(1u, SPLIT_LDS_WORDS / ld);
    const uint32_t grid = std::max(1u, std::min((n_rows + batch - 1) / batch, n_cu * 2u));
    const size_t lds = (size_t)batch * ld * 4;
    uint32_t* w = reinterpret_cast<uint32_t*>(rows);
    if (forward) hipLaunchKernelGGL(row_split_kernel<true>, dim3(grid), dim3(SPLIT_THREADS), lds, s, w, ld, n_rows, batch, nonfinite);
    else hipLaunchKernelGGL(row_split_kernel<false>, dim3(grid), dim3(SPLIT_THREADS), lds, s, w, ld, n_rows, batch, nonfinite);
}

}  // namespace vdb

// row_split.h -- the codec of the SPLIT row layout, for host and device code alike.
//
// A stored row keeps its address and its pitch of 4 * ld bytes in both layouts.  F32: ld floats.  SPLIT: bytes [0, 2 ld) hold
// one 16-bit HI word per element, bytes [2 ld, 4 ld) the element's LO word.  With `bits` the f32 pattern of the element,
//     lo = bits & 0xffff
//     hi = ((bits >> 16) + (lo >> 15)) & 0xffff         upper = (hi - (lo >> 15)) & 0xffff
// a 16-bit modular add of the one bit both sides can see, hence a bijection on all 2^32 patterns: every reader that wants the
// f32 value gets it back exactly.  hi, read as bf16, is the element rounded HALF UP IN MAGNITUDE (fused_bf16_common.h says why
// the screening tier may read that in the place of the round-to-nearest-even value), so the filter pass streams the hi plane
// of a row -- 2 bytes per element -- and nothing else.  Zero encodes to zero: the zero-filled rows past the last one and the
// padding columns look the same in both layouts.
//
// The add wraps for the patterns whose upper half is 0x7fff or 0xffff with bit 15 set (two NaN families, 0xffffffff among
// them): their hi word reads as +-0.  The forward conversion reports every element with an all-ones exponent and the index
// then stays F32, so no reader ever scores such a word.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VDB_SPLIT_HD __host__ __device__ inline
#else
#define VDB_SPLIT_HD inline
#endif

namespace vdb {

constexpr int LAYOUT_F32 = 0, LAYOUT_SPLIT = 1;

VDB_SPLIT_HD uint32_t split_lo(uint32_t bits) { return bits & 0xffffu; }
VDB_SPLIT_HD uint32_t split_hi(uint32_t bits) { return ((bits >> 16) + ((bits >> 15) & 1u)) & 0xffffu; }
VDB_SPLIT_HD uint32_t split_join(uint32_t hi, uint32_t lo) { return (((hi - (lo >> 15)) & 0xffffu) << 16) | lo; }
VDB_SPLIT_HD bool split_nonfinite(uint32_t bits) { return (bits & 0x7f800000u) == 0x7f800000u; }

// Two elements at a time, as the kernels hold them: hi2 / lo2 carry element 2i in their low half and element 2i + 1 in their
// high half.  The halves never borrow from each other (16-bit lanes).
VDB_SPLIT_HD void split_pack2(uint32_t b0, uint32_t b1, uint32_t* hi2, uint32_t* lo2) {
    *hi2 = split_hi(b0) | (split_hi(b1) << 16);
    *lo2 = split_lo(b0) | (split_lo(b1) << 16);
}
VDB_SPLIT_HD void split_join2(uint32_t hi2, uint32_t lo2, uint32_t* b0, uint32_t* b1) {
    const uint32_t carry = (lo2 >> 15) & 0x00010001u;
    const uint32_t up = (((hi2 & 0xffffu) - (carry & 0xffffu)) & 0xffffu) | ((hi2 & 0xffff0000u) - (carry & 0xffff0000u));
    *b0 = (up << 16) | (lo2 & 0xffffu);
    *b1 = (up & 0xffff0000u) | (lo2 >> 16);
}

}  // namespace vdb

// The codec of the SPLIT row layout (vectordb-from-scratch_amd/csrc/row_split.h) on the CPU:
//   1. encode then decode is the identity -- on the patterns where a modular add could go wrong, on 10^7 random ones, and through
//      the two-at-a-time forms the kernels use;
//   2. for EVERY finite f32 pattern the hi word, read as bf16, is within half a bf16 ulp of the value, or it is +-inf exactly
//      where round-to-nearest-even is +-inf; it differs from the RNE value only on ties (lo == 0x8000);
//   3. zero encodes to zero and the wrapping NaN families are the ones the header names.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "row_split.h"

using namespace vdb;

static int failures = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (failures++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                  \
    } while (0)

static bool round_trip(uint32_t bits) {
    const uint32_t hi = split_hi(bits), lo = split_lo(bits);
    if (hi > 0xffffu || lo > 0xffffu) return false;
    if (split_join(hi, lo) != bits) return false;
    // the packed forms, with the pattern in either half and an awkward neighbour in the other
    const uint32_t other[3] = {0u, 0xffffffffu, 0x7f7f8000u};
    for (uint32_t o : other) {
        uint32_t h2, l2, b0, b1;
        split_pack2(bits, o, &h2, &l2);
        split_join2(h2, l2, &b0, &b1);
        if (b0 != bits || b1 != o) return false;
        split_pack2(o, bits, &h2, &l2);
        split_join2(h2, l2, &b0, &b1);
        if (b0 != o || b1 != bits) return false;
    }
    return true;
}

static uint32_t rne_bf16(uint32_t bits) { return (bits + 0x7fffu + ((bits >> 16) & 1u)) >> 16; }   // finite inputs only

static double as_double(uint32_t f32_bits) {
    float f;
    memcpy(&f, &f32_bits, 4);
    return (double)f;
}

// finite patterns [begin, end): the half-ulp bound, the infinities, the ties
static void check_range(uint64_t begin, uint64_t end, std::atomic<uint64_t>* bad, std::atomic<uint64_t>* ties, std::atomic<uint64_t>* infs) {
    uint64_t nbad = 0, nties = 0, ninf = 0;
    for (uint64_t v = begin; v < end; ++v) {
        const uint32_t bits = (uint32_t)v;
        if (split_nonfinite(bits)) continue;
        const uint32_t hi = split_hi(bits), rne = rne_bf16(bits);
        const bool hi_inf = (hi & 0x7fffu) == 0x7f80u, rne_inf = (rne & 0x7fffu) == 0x7f80u;
        if (hi_inf != rne_inf) { ++nbad; continue; }
        if ((hi & 0x8000u) != (bits >> 31 << 15)) { ++nbad; continue; }          // the sign never changes
        if (hi_inf) { ++ninf; continue; }
        // half a bf16 ulp of x: bf16 keeps 8 significant bits, so ulp = 2^(e - 7) with e the exponent of x (-126 for denormals)
        const uint32_t ef = (bits >> 23) & 0xffu;
        const int e = ef ? (int)ef - 127 : -126;
        uint64_t half_bits = (uint64_t)(e - 8 + 1023) << 52;
        double half_ulp;
        memcpy(&half_ulp, &half_bits, 8);
        const double err = std::fabs(as_double(bits) - as_double(hi << 16));
        if (!(err <= half_ulp)) ++nbad;
        if (hi != rne) {
            if (split_lo(bits) != 0x8000u) ++nbad;                               // only a tie may round the other way
            ++nties;
        }
    }
    *bad += nbad; *ties += nties; *infs += ninf;
}

int main() {
    // ---- 1. identity on the listed patterns
    const uint32_t los[6] = {0u, 1u, 0x7fffu, 0x8000u, 0x8001u, 0xffffu};
    for (uint32_t sign = 0; sign < 2; ++sign)
        for (uint32_t ef = 0; ef < 256; ++ef)                                    // every exponent, denormals and the all-ones one included
            for (uint32_t mant7 : {0u, 1u, 0x3fu, 0x7eu, 0x7fu})
                for (uint32_t lo : los) {
                    const uint32_t bits = (sign << 31) | (ef << 23) | (mant7 << 16) | lo;
                    CHECK(round_trip(bits), "round trip of %08x", bits);
                }
    for (uint32_t upper : {0x0000u, 0x8000u, 0x0001u, 0x8001u, 0x007fu, 0x7f7fu, 0x7f80u, 0x7fffu, 0xff7fu, 0xff80u, 0xffffu})
        for (uint32_t lo = 0; lo < 0x10000u; ++lo) CHECK(round_trip((upper << 16) | lo), "round trip of %04x%04x", upper, lo);
    std::mt19937_64 rng(12345);
    for (int i = 0; i < 10000000; ++i) {
        const uint32_t bits = (uint32_t)rng();
        if (!round_trip(bits)) { CHECK(false, "round trip of random %08x", bits); break; }
    }
    // ---- 3. zero, and the families that wrap
    CHECK(split_hi(0u) == 0u && split_lo(0u) == 0u, "+0 encodes to zero");
    CHECK(split_hi(0x80000000u) == 0x8000u && split_lo(0x80000000u) == 0u, "-0 keeps its pattern");
    CHECK(split_hi(0xffffffffu) == 0x0000u && split_hi(0x7fff8000u) == 0x8000u, "the wrapping NaN families read as zeros");
    CHECK(split_nonfinite(0xffffffffu) && split_nonfinite(0x7f800000u) && split_nonfinite(0xff800001u) && !split_nonfinite(0x7f7fffffu) &&
              !split_nonfinite(0u) && !split_nonfinite(0x00000001u),
          "the all-ones exponent is what the forward conversion reports");
    for (uint64_t v = 0; v < (1ull << 32); v += 4099) {                          // a wrapped hi word is always a non-finite element
        const uint32_t bits = (uint32_t)v, up = bits >> 16;
        if (((up + ((bits >> 15) & 1u)) >> 16) != 0) CHECK(split_nonfinite(bits), "%08x wraps but is finite", bits);
    }
    // ---- 2. every finite pattern
    std::atomic<uint64_t> bad{0}, ties{0}, infs{0};
    const unsigned nt = 8;
    std::vector<std::thread> th;
    const uint64_t total = 1ull << 32, step = total / nt;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(check_range, t * step, t == nt - 1 ? total : (t + 1) * step, &bad, &ties, &infs);
    for (auto& t : th) t.join();
    CHECK(bad.load() == 0, "%llu finite patterns break the half-ulp bound, the infinities or the tie rule", (unsigned long long)bad.load());
    // ties that RNE sends DOWN (even upper half) are the ones that differ: half of the 2 x 0x7f80 finite upper halves, minus none
    CHECK(ties.load() == 2ull * 0x7f80u / 2, "%llu patterns differ from RNE", (unsigned long long)ties.load());
    CHECK(infs.load() == 2ull * 0x8000u, "%llu finite patterns round to an infinity", (unsigned long long)infs.load());
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("row split ok: %llu ties differ from RNE, %llu finite patterns reach an infinity\n", (unsigned long long)ties.load(), (unsigned long long)infs.load());
    return 0;
}

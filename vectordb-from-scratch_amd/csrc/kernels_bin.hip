// kernels_bin.hip -- the binary flat index (include/vdb_flat.h "Binary vectors"): exact Hamming / Jaccard top-k
// on the integer matrix cores of gfx950.  Rows stay PACKED in HBM at 1 bit per element; a = popcount(q & x) is the dot product of
// two 0/1 byte vectors on v_mfma_i32_16x16x64_i8, exact in i32; h = nq + nx - 2a and u = nq + nx - a follow from the popcounts.
//
//   widen   once per call: every query of the batch from packed bits to one 0/1 byte per bit in HBM, in the K order below, so that
//           staging a query tile into LDS is a plain copy.
//   score   ONE workgroup of 512 threads (8 waves) per (segment of R consecutive rows, tile of QT queries).  A wave owns 32 rows of
//           a round of 256: two A operands.  Lane (row r = lane & 15, group g = lane >> 4) takes ONE 16-byte load of packed bytes
//           [16g, 16g + 16) of a 64-byte (512-bit) chunk of row r and feeds EIGHT K steps from it: step j widens the lane's bits
//           [16j, 16j + 16) to 16 bytes in registers (bit field extract, a 24-bit multiply that spreads 4 bits to 4 bytes, a mask:
//           3 VALU per operand dword, 24 per wave and step for both row blocks, against 2 x QT/16 MFMAs).  The matrix unit does not
//           care which bit sits at which K position as long as both operands agree, and the query image is widened by the same
//           function in the same order.  The next chunk's loads -- the next round's first chunk after the last -- are in flight
//           under this chunk's MFMAs.  Workgroup ids are re-ordered so that the tiles of a segment share an XCD's L2.
//   select  built for integer scores:
//           1. one u32 per query in HBM holds the f32 bits of the best k-th distance any workgroup has proven (atomicMin after a
//              prune; read relaxed at the start of every round); it outlives the segment;
//           2. the accumulators are tested in registers against min(shared, own) threshold -- under Hamming one shift-subtract and
//              one integer compare -- and only survivors look up the live bit, the mask and the id rank and form a key;
//           3. survivors take a slot of the query's LDS buffer with an LDS atomic.  A round ends WITHOUT a barrier: the waves run
//              free.  A wave whose offer found its buffer full raises a flag in LDS and waits at the barrier of a prune episode;
//              the others see the flag at the end of their round (or come when their rows are done) and join; the episode sorts the
//              buffers that grew, cuts them to k, publishes the thresholds.  (Where the image holds only a part of a query and is
//              re-staged with barriers, the waves are in lockstep anyway and the round ends in one __syncthreads_or.)
//   merge   one workgroup per query streams the segments' partial lists through the select of kernels_spv_select.h.
// Compiled with -ffp-contract=off; every f32 operation of a distance is one correctly rounded IEEE operation.
#include "kernels.h"
#include "kernels_bin.h"
#include "kernels_spv_select.h"

#pragma clang fp contract(off)

namespace vdb {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr uint32_t BIN_WAVES = BIN_THREADS / 64;
constexpr int32_t BIN_NO_ROW = 1 << 24;             // the popcount of a row that does not exist: no threshold lets it pass under Hamming

// the f32 bits of the distance; d >= +0, so the bits order as the distances do
template <int METRIC> __device__ __forceinline__ uint32_t bin_distance_bits(int32_t a, int32_t nq, int32_t nx) {
    if (METRIC == BIN_HAMMING) return __float_as_uint((float)(nq + nx - 2 * a));
    const int32_t u = nq + nx - a;
    return u == 0 ? 0u : __float_as_uint(__fsub_rn(1.0f, __fdiv_rn((float)a, (float)u)));
}

// 16 bits of `word` from bit `sh` to one 0/1 byte per bit: dword w holds bits [4w, 4w + 4), byte b of it bit 4w + b.
// x * 0x204081 puts bit i of a 4-bit x at position 8i (and others in between, without a carry); the mask keeps those four.
template <int SH> __device__ __forceinline__ v4i bin_widen16(uint32_t word) {
    v4i r;
#pragma unroll
    for (int w = 0; w < 4; ++w) r[w] = (int)(__umul24(__builtin_amdgcn_ubfe(word, SH + 4 * w, 4), 0x204081u) & 0x01010101u);
    return r;
}

// ---- the popcounts of added rows: one wave per row
__global__ __launch_bounds__(256) void bin_row_popcounts_kernel(const uint8_t* __restrict__ rows, uint32_t ld, uint32_t row_begin, uint32_t row_end,
                                                                int32_t* __restrict__ nx) {
    const uint32_t lane = threadIdx.x & 63, row = row_begin + blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= row_end) return;                      // (whole waves leave: no barrier follows)
    const uint8_t* __restrict__ x = rows + (size_t)row * ld;
    int32_t sum = 0;
    for (uint32_t off = lane * 16; off < ld; off += 64 * 16) {        // ld is a multiple of 64: a piece is inside the row
        const v4i v = *reinterpret_cast<const v4i*>(x + off);
        for (int w = 0; w < 4; ++w) sum += __popc((uint32_t)v[w]);
    }
    for (uint32_t d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    if (lane == 0) nx[row] = sum;
}

__global__ __launch_bounds__(256) void bin_fill_kernel(uint32_t* __restrict__ words, size_t n, uint32_t value) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) words[i] = value;
}

// ---- the batch's queries, widened: piece (chunk, step j, group g) of 16 bytes is packed bytes 64 chunk + 16 g + 2 j and + 1
__global__ __launch_bounds__(256) void bin_widen_kernel(const uint8_t* __restrict__ q, uint32_t ld, size_t pieces, uint8_t* __restrict__ qw) {
    const uint32_t per_query = ld >> 1;              // 16-byte pieces of one widened query: 8 ld / 16
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < pieces; i += (size_t)gridDim.x * blockDim.x) {
        const size_t b = i / per_query;
        const uint32_t pc = (uint32_t)(i - b * per_query), chunk = pc >> 5, j = (pc >> 2) & 7, g = pc & 3;
        const uint8_t* src = q + b * ld + 64 * chunk + 16 * g + 2 * j;
        *reinterpret_cast<v4i*>(qw + i * 16) = bin_widen16<0>((uint32_t)src[0] | ((uint32_t)src[1] << 8));
    }
}

// ---- a prune episode's network.  Every buffer that has grown to k or more keys since it was last sorted is sorted ascending by ONE
// bitonic network whose comparators all point upwards -- slots at and above a buffer's fill count as +inf and never move, so a
// buffer needs no power-of-two room -- and cut to its k smallest keys; the k-th becomes the query's threshold here and, by
// atomicMin on its distance bits, a bound for every other workgroup of the launch.  Called by the whole workgroup.
template <uint32_t QT>
__device__ inline void bin_prune(uint64_t* s_keys, uint64_t* s_thr, uint32_t* s_cnt, const uint32_t* s_kq, uint32_t* s_need, uint32_t* s_sorted,
                                 uint32_t cap, uint32_t P, uint32_t* gthr) {
    const uint32_t tid = threadIdx.x;
    if (tid < QT) {
        const uint32_t kq = s_kq[tid], capq = min(cap, bin_select_cap(kq)), n = min(s_cnt[tid], capq);
        s_cnt[tid] = n;                              // (offers that found no room counted themselves in)
        s_need[tid] = kq && n >= kq && n > s_sorted[tid];
    }
    __syncthreads();
    const uint32_t half = P >> 1, lh = __ffs(half) - 1;   // every size here is a power of two: shifts and masks, no division
    for (uint32_t k2 = 2; k2 <= P; k2 <<= 1)
        for (uint32_t j = k2 >> 1, lj = __ffs(j) - 1; j > 0; j >>= 1, --lj) {
            for (uint32_t item = tid; item < QT * half; item += BIN_THREADS) {
                const uint32_t q = item >> lh, pi = item & (half - 1);
                if (!s_need[q]) continue;
                const uint32_t blk = pi >> lj, off = pi & (j - 1);
                uint32_t i, o;
                if (j == (k2 >> 1)) { i = blk * k2 + off; o = i + k2 - 1 - 2 * off; }   // the mirror step of a merge
                else { i = blk * 2 * j + off; o = i + j; }
                if (o < s_cnt[q]) {                  // o < fill <= capq <= cap: inside the buffer
                    uint64_t* kk = s_keys + (size_t)q * cap;
                    const uint64_t x = kk[i], y = kk[o];
                    if (x > y) { kk[i] = y; kk[o] = x; }
                }
            }
            __syncthreads();
        }
    if (tid < QT && s_need[tid]) {
        const uint32_t kq = s_kq[tid];
        const uint64_t kth = s_keys[(size_t)tid * cap + kq - 1];
        s_cnt[tid] = kq; s_sorted[tid] = kq; s_thr[tid] = kth;
        atomicMin(&gthr[tid], (uint32_t)(kth >> 32));        // kq eligible rows at or below it exist (kq > 0 only for a query of the launch)
    }
    __syncthreads();
}

// one 512-bit chunk: eight K steps, each widening 16 bits of both row blocks and multiplying them with every query block
template <int QB, int J>
__device__ __forceinline__ void bin_step(const v4i (&x)[2], const unsigned char* bp, uint32_t stride, v4i (&acc)[2][QB]) {
    const v4i a0 = bin_widen16<16 * (J & 1)>((uint32_t)x[0][J >> 1]), a1 = bin_widen16<16 * (J & 1)>((uint32_t)x[1][J >> 1]);
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const v4i b = *reinterpret_cast<const v4i*>(bp + qb * 16 * stride + 64 * J);
        acc[0][qb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b, acc[0][qb], 0, 0, 0);
        acc[1][qb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b, acc[1][qb], 0, 0, 0);
    }
}
template <int QB>
__device__ __forceinline__ void bin_chunk(const v4i (&x)[2], const unsigned char* bp, uint32_t stride, v4i (&acc)[2][QB]) {
    bin_step<QB, 0>(x, bp, stride, acc); bin_step<QB, 1>(x, bp, stride, acc); bin_step<QB, 2>(x, bp, stride, acc); bin_step<QB, 3>(x, bp, stride, acc);
    bin_step<QB, 4>(x, bp, stride, acc); bin_step<QB, 5>(x, bp, stride, acc); bin_step<QB, 6>(x, bp, stride, acc); bin_step<QB, 7>(x, bp, stride, acc);
}

// ---- score + select
template <int QB, int METRIC>
__global__ __launch_bounds__(BIN_THREADS) void bin_score_kernel(BinSearchParams p) {
    constexpr uint32_t QT = 16 * QB;
    extern __shared__ __attribute__((aligned(16))) unsigned char s_img[];   // [QT][stride]
    const uint32_t stride = p.kc + 16;               // bytes between two queries of the image: an odd number of 16-byte groups
    uint64_t* s_keys = reinterpret_cast<uint64_t*>(s_img + QT * stride);      // [QT][cap]
    uint64_t* s_thr = s_keys + (size_t)QT * p.cap;   // the k-th key of a buffer that has been cut, EMPTY_KEY before
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_thr + QT);
    uint32_t* s_kq = s_cnt + QT;
    uint32_t* s_need = s_kq + QT;
    uint32_t* s_sorted = s_need + QT;
    uint32_t* s_capq = s_sorted + QT;
    int32_t* s_nq = reinterpret_cast<int32_t*>(s_capq + QT);
    uint32_t* s_kmax = reinterpret_cast<uint32_t*>(s_nq + QT);
    uint32_t* s_flag = s_kmax + 1;                   // some wave waits for a prune episode
    uint32_t* s_done = s_kmax + 2;                   // waves that have scored all their rows
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
    // Workgroup ids go round the 8 XCDs; this order gives every XCD a run of consecutive (segment, tile) pairs, so that the tiles of
    // one segment meet its rows in one L2.  The grid is padded to a multiple of 8: the surplus leaves here.
    const uint32_t tiles = (p.n_q + QT - 1) / QT, wg = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    if (wg >= p.segs * tiles) return;
    const uint32_t seg = wg / tiles, y0 = (wg - seg * tiles) * QT;
    const uint32_t r0 = seg * p.seg_rows, nr = min(p.seg_rows, p.n_rows - r0), rend = r0 + nr;   // seg < segs = ceil(n_rows / seg_rows)
    const uint32_t ld = p.ld, cap = p.cap;
    uint32_t* gthr = p.gthr + y0;                    // indexed below by queries of the launch only
    if (tid == 0) { *s_kmax = 0; *s_flag = 0; *s_done = 0; }
    __syncthreads();
    if (tid < QT) {
        const bool valid = y0 + tid < p.n_q;
        const uint32_t kq = valid ? min(p.ks[p.q0 + y0 + tid], min(p.kout, BIN_MAX_K)) : 0;
        s_kq[tid] = kq; s_cnt[tid] = 0; s_sorted[tid] = 0; s_thr[tid] = EMPTY_KEY;
        s_capq[tid] = min(cap, bin_select_cap(kq));
        s_nq[tid] = valid ? p.nq[p.q0 + y0 + tid] : 0;
        atomicMax(s_kmax, kq);
    }
    __syncthreads();
    uint32_t P = 2;                                  // the network's size: the largest buffer of the tile
    while (P < min(cap, bin_select_cap(*s_kmax))) P <<= 1;

    // one prune episode; true when every wave has scored all its rows (s_done moves only outside an episode).
    // RELIANCE: where the waves run free, the eight waves reach an episode's barriers from DIFFERENT program points (the offer
    // loop of any round, the tail loop below).  That is sound on this hardware -- a workgroup has one barrier that counts arriving
    // waves, whatever their program counter -- but HIP does not promise it for barriers in control flow the compiler cannot prove
    // uniform; every condition that guards an episode is therefore made wave-uniform by a ballot or a readfirstlane.  Two
    // invariants keep the count right and must survive any change: every wave is inside an episode or none is (a wave enters
    // only at the episode's first barrier and leaves only after bin_prune's last), and NO wave may return before the episode
    // that reports all eight done.
    auto episode = [&]() -> bool {
        __syncthreads();                             // every wave is here, every offer it made is in its buffer
        const bool all = __builtin_amdgcn_readfirstlane(*(volatile uint32_t*)s_done) == BIN_WAVES;
        if (tid == 0) *s_flag = 0;
        bin_prune<QT>(s_keys, s_thr, s_cnt, s_kq, s_need, s_sorted, cap, P, gthr);
        return all;
    };

    const uint32_t wide = 8 * ld, chunks = (wide + p.kc - 1) / p.kc, row_chunks = ld >> 6;
    const uint32_t rounds = (nr + BIN_ROUND_ROWS - 1) / BIN_ROUND_ROWS;
    const bool lockstep = chunks > 1;                // the image is re-staged between barriers: the waves cannot run free
    // the lane's operand row of block rb in round it; a row beyond the store is read as the last row and never offered
    auto row_ptr = [&](uint32_t it, uint32_t rb) {
        return p.rows + (size_t)min(r0 + it * BIN_ROUND_ROWS + wave * 32 + 16 * rb + c, p.n_rows - 1) * ld + 16 * g;
    };
    v4i cur[2], nxt[2];
    cur[0] = *reinterpret_cast<const v4i*>(row_ptr(0, 0));
    cur[1] = *reinterpret_cast<const v4i*>(row_ptr(0, 1));
    nxt[0] = cur[0]; nxt[1] = cur[1];
    for (uint32_t it = 0; it < rounds; ++it) {
        const uint32_t base = r0 + it * BIN_ROUND_ROWS + wave * 32;
        const uint8_t* __restrict__ x0 = row_ptr(it, 0);
        const uint8_t* __restrict__ x1 = row_ptr(it, 1);
        // what the pre-test needs, asked for now: it arrives under the K loop.  The popcounts of the lane's 8 result rows
        // (base + 16 rb + 4 g + r) and the shared thresholds of its QB queries (16 qb + c), read relaxed: a stale one is merely weaker
        int32_t nxv[8];
        uint32_t gt[QB];
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            const uint32_t row = base + 16 * (rr >> 2) + 4 * g + (rr & 3);
            nxv[rr] = row < rend ? p.nx[row] : BIN_NO_ROW;
        }
#pragma unroll
        for (int qb = 0; qb < QB; ++qb)
            gt[qb] = y0 + 16 * qb + c < p.n_q ? __atomic_load_n(&gthr[16 * qb + c], __ATOMIC_RELAXED) : BIN_OPEN;
        v4i acc[2][QB];
        for (int rb = 0; rb < 2; ++rb)
            for (int qb = 0; qb < QB; ++qb) acc[rb][qb] = v4i{0, 0, 0, 0};
        for (uint32_t ch = 0; ch < chunks; ++ch) {
            const uint32_t kc0 = ch * p.kc, kc_len = min(p.kc, wide - kc0);         // a multiple of 512
            if (lockstep || it == 0) {               // (uniform) the image: once where a query fits, else per round and chunk
                __syncthreads();                     // nobody reads the chunk before any more
                const uint32_t pieces = kc_len >> 4;
                for (uint32_t i = tid; i < QT * pieces; i += BIN_THREADS) {
                    const uint32_t q = i / pieces, pc = i - q * pieces;
                    v4i v = v4i{0, 0, 0, 0};
                    if (y0 + q < p.n_q) v = *reinterpret_cast<const v4i*>(p.qw + (size_t)(p.q0 + y0 + q) * wide + kc0 + 16 * pc);
                    *reinterpret_cast<v4i*>(s_img + q * stride + 16 * pc) = v;
                }
                __syncthreads();
            }
            const unsigned char* bp = s_img + c * stride + 16 * g;
            const uint32_t gc0 = kc0 >> 9, nch = kc_len >> 9;
            for (uint32_t cc = 0; cc < nch; ++cc) {
                const uint32_t gc = gc0 + cc;        // the row's chunk; its successor -- the next round's first -- is asked for first
                if (gc + 1 < row_chunks) {
                    nxt[0] = *reinterpret_cast<const v4i*>(x0 + 64 * (gc + 1));
                    nxt[1] = *reinterpret_cast<const v4i*>(x1 + 64 * (gc + 1));
                } else if (it + 1 < rounds) {
                    nxt[0] = *reinterpret_cast<const v4i*>(row_ptr(it + 1, 0));
                    nxt[1] = *reinterpret_cast<const v4i*>(row_ptr(it + 1, 1));
                }
                bin_chunk<QB>(cur, bp + 512 * cc, stride, acc);
                cur[0] = nxt[0]; cur[1] = nxt[1];
            }
        }

        // ---- the pre-test, in registers: the lane holds rows base + 16 rb + 4 g + r against queries 16 qb + c
        int32_t tbs[QB], nqv[QB], hm[QB];            // tbs: the threshold's distance bits as a signed number, -1 for a query that takes nothing
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            const uint32_t q = 16 * qb + c, t = min(gt[qb], (uint32_t)(s_thr[q] >> 32));
            tbs[qb] = s_kq[q] ? (int32_t)min(t, 0x7fffffffu) : -1;
            nqv[qb] = s_nq[q];
            // Hamming: h <= floor(t)  <=>  2a - nx >= nq - floor(t); an open threshold admits every h (<= 32768) of a row that exists
            const int32_t ti = tbs[qb] < 0 ? -1 : tbs[qb] == 0x7fffffff ? (1 << 20) : (int32_t)__int_as_float(tbs[qb]);
            hm[qb] = nqv[qb] - ti;
        }
        uint32_t pending = 0;
#pragma unroll
        for (int rr = 0; rr < 8; ++rr)
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                const int32_t a = acc[rr >> 2][qb][rr & 3];
                const bool pass = METRIC == BIN_HAMMING ? 2 * a - nxv[rr] >= hm[qb]
                                                        : (int32_t)bin_distance_bits<METRIC>(a, nqv[qb], nxv[rr]) <= tbs[qb];
                pending |= (uint32_t)pass << (rr * QB + qb);
            }
        // ---- survivors only: the row's existence, live bit, mask bit and id rank
        uint32_t rk[8];
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            rk[rr] = 0;
            const uint32_t of_row = ((1u << QB) - 1u) << (rr * QB);
            if (pending & of_row) {
                const uint32_t row = base + 16 * (rr >> 2) + 4 * g + (rr & 3);
                bool ok = row < rend;
                if (ok) ok = (p.live[row >> 5] >> (row & 31)) & 1u;
                if (ok && p.id_mask) {
                    const uint64_t id = p.row_ids[row];
                    ok = id < p.mask_bits && ((p.id_mask[id >> 6] >> (id & 63)) & 1ull);
                }
                if (ok) rk[rr] = p.rank[row];
                else pending &= ~of_row;
            }
        }
        for (;;) {
            if (pending) {
                uint32_t still = 0;
#pragma unroll
                for (int rr = 0; rr < 8; ++rr)
#pragma unroll
                    for (int qb = 0; qb < QB; ++qb) {
                        const uint32_t bit = 1u << (rr * QB + qb);
                        if (pending & bit) {
                            const uint32_t q = 16 * qb + c;
                            const uint64_t key = ((uint64_t)bin_distance_bits<METRIC>(acc[rr >> 2][qb][rr & 3], nqv[qb], nxv[rr]) << 32) | rk[rr];
                            if (key < s_thr[q]) {    // (keys are unique: the k-th key itself is in the buffer)
                                const uint32_t slot = atomicAdd(&s_cnt[q], 1u);
                                if (slot < s_capq[q]) s_keys[(size_t)q * cap + slot] = key;   // capq <= cap: inside the query's buffer
                                else still |= bit;   // the buffer is full: pruned below, offered again
                            }
                        }
                    }
                pending = still;
            }
            const bool mine = __ballot(pending != 0) != 0;   // (uniform in the wave)
            bool join;
            if (lockstep) join = __syncthreads_or(pending != 0);
            else {
                if (mine && lane == 0) *(volatile uint32_t*)s_flag = 1;
                join = mine || __builtin_amdgcn_readfirstlane(*(volatile uint32_t*)s_flag) != 0;
            }
            if (!join) break;
            episode();
            if (!lockstep && !mine) break;           // (in lockstep every wave goes round again and leaves through the vote)
        }
    }
    // the wave's rows are done; episodes until every wave's are (the last one leaves every buffer at or below its k)
    if (lane == 0) atomicAdd(s_done, 1u);
    while (!episode()) {}
    for (uint32_t q = wave; q < QT; q += BIN_WAVES) {
        if (y0 + q >= p.n_q) continue;               // (uniform in the wave)
        const size_t slot = (size_t)(y0 + q) * p.segs + seg;
        const uint32_t cnt = s_cnt[q];               // <= k of the query <= kout
        for (uint32_t i = lane; i < cnt; i += 64) p.part[slot * p.kout + i] = s_keys[(size_t)q * cap + i];
        if (lane == 0) p.part_cnt[slot] = cnt;
    }
    if (tid < 64) {
        uint32_t v = (tid < QT && y0 + tid < p.n_q) ? s_cnt[tid] : 0;
        for (uint32_t d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
        if (tid == 0 && v) atomicAdd(&p.counters[0], (unsigned long long)v);
    }
}

// ---- merge: one workgroup of SPV_THREADS per query; the key's high word is the distance's own bits
__global__ __launch_bounds__(SPV_THREADS) void bin_merge_kernel(BinSearchParams p) {
    __shared__ uint64_t s_keys[SPV_SELECT_CAP];
    __shared__ uint64_t s_thr;
    __shared__ uint32_t s_cnt;
    const uint32_t tid = threadIdx.x, y = blockIdx.x, b = p.q0 + y;
    if (tid == 0) { s_cnt = 0; s_thr = EMPTY_KEY; }
    __syncthreads();
    const uint32_t kq = min(p.ks[b], min(p.kout, BIN_MAX_K));
    const uint64_t* __restrict__ part = p.part + (size_t)y * p.segs * p.kout;
    const uint32_t* __restrict__ part_cnt = p.part_cnt + (size_t)y * p.segs;
    const uint64_t total = (uint64_t)p.segs * p.kout;
    uint32_t bound = 0;
    for (uint64_t j = tid; j - tid < total; j += SPV_THREADS) {
        if (bound + SPV_THREADS > SPV_SELECT_CAP) bound = spv_prune(s_keys, &s_cnt, &s_thr, kq);
        int pushed = 0;
        if (j < total) {
            const uint64_t seg = j / p.kout;
            if ((uint32_t)(j - seg * p.kout) < part_cnt[seg]) {      // a slot its workgroup has written
                const uint64_t key = part[j];
                pushed = key < s_thr;
                spv_offer(s_keys, &s_cnt, &s_thr, key);               // below bound + SPV_THREADS <= SPV_SELECT_CAP
            }
        }
        bound += (uint32_t)__syncthreads_count(pushed);
    }
    const uint32_t cnt = spv_prune(s_keys, &s_cnt, &s_thr, kq);
    for (uint32_t i = tid; i < cnt; i += SPV_THREADS) {
        const uint64_t key = s_keys[i];
        p.out_ids[(size_t)b * p.kout + i] = p.sorted_ids[(uint32_t)key];
        p.out_dists[(size_t)b * p.kout + i] = __uint_as_float((uint32_t)(key >> 32));
    }
    if (tid == 0) p.out_counts[b] = cnt;
}

template <int QB> void launch_score(const BinSearchParams& p, uint32_t grid, size_t lds, hipStream_t s) {
    if (p.metric == BIN_HAMMING) hipLaunchKernelGGL((bin_score_kernel<QB, BIN_HAMMING>), dim3(grid), dim3(BIN_THREADS), lds, s, p);
    else hipLaunchKernelGGL((bin_score_kernel<QB, BIN_JACCARD>), dim3(grid), dim3(BIN_THREADS), lds, s, p);
}

size_t score_lds(size_t qt, uint32_t kc, uint32_t cap) { return qt * (kc + 16) + qt * (size_t)cap * 8 + qt * (8 + 6 * 4) + 16; }

}  // namespace

void launch_bin_row_popcounts(const uint8_t* rows, uint32_t ld, uint32_t row_begin, uint32_t row_end, int32_t* nx, hipStream_t s) {
    if (row_end <= row_begin) return;
    hipLaunchKernelGGL(bin_row_popcounts_kernel, dim3((row_end - row_begin + 3) / 4), dim3(256), 0, s, rows, ld, row_begin, row_end, nx);
}

void launch_bin_fill(uint32_t* words, size_t n, uint32_t value, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(bin_fill_kernel, dim3((uint32_t)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, s, words, n, value);
}

void launch_bin_widen(const uint8_t* q, uint32_t ld, size_t nq, uint8_t* qw, hipStream_t s) {
    const size_t pieces = nq * (ld >> 1);
    if (!pieces) return;
    hipLaunchKernelGGL(bin_widen_kernel, dim3((uint32_t)std::min<size_t>((pieces + 255) / 256, 4096)), dim3(256), 0, s, q, ld, pieces, qw);
}

void launch_bin_score(const BinSearchParams& p, hipStream_t s) {
    if (!p.n_q || !p.segs) return;
    const uint32_t tiles = (p.n_q + p.qt - 1) / p.qt;                 // the host keeps segs * tiles below 2^31
    // the image holds as much of every widened query as the select buffers leave of the LDS budget (at least one 512-byte chunk:
    // the largest buffers, 16 x 1088 keys, leave 1264 bytes per query), at most the whole query
    BinSearchParams q = p;
    q.kc = std::min<uint32_t>(8 * p.ld, (uint32_t)((BIN_LDS_BUDGET - score_lds(p.qt, 0, p.cap)) / p.qt) / 512 * 512);
    const uint32_t grid = (p.segs * tiles + 7) / 8 * 8;
    const size_t lds = score_lds(p.qt, q.kc, p.cap);
    if (p.qt == BIN_QT) launch_score<BIN_QT / 16>(q, grid, lds, s);
    else launch_score<BIN_QT_LARGE_K / 16>(q, grid, lds, s);
}

void launch_bin_merge(const BinSearchParams& p, hipStream_t s) {
    if (!p.n_q) return;
    hipLaunchKernelGGL(bin_merge_kernel, dim3(p.n_q), dim3(SPV_THREADS), 0, s, p);
}

}  // namespace vdb

// kernels_sparse_tile_body.h -- the body of an eligible-row scan kernel: one 64 x 64 tile of (list position, query) pairs,
// staged through LDS, every pair ONE sequential left fold in the reference's operation order, the metric's epilogue, the keys
// stored through LDS.  Textually included INSIDE a 256-thread __global__ function template <bool EUC> that has
//     SparseScanParams p          the scan as the tile sees it: p.elig / p.n_elig the list, queries below p.nq exist
//     SPARSE_TILE_J0              first list position of the workgroup's tile (workgroup-uniform, a multiple of 64)
//     SPARSE_TILE_Q0              first query of the tile (workgroup-uniform)
// in scope, so that both kernels run the same statements: the fold exists once, and the code generated for the older kernel
// is the code it had before the newer one existed.  No include guard on purpose.
    __shared__ __attribute__((aligned(16))) float sImg[2 * SP_IMG];
    __shared__ uint32_t sRow[SP_TR];

    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t j0 = SPARSE_TILE_J0;                       // first list position of the tile
    const uint32_t q0 = SPARSE_TILE_Q0;                       // first query (of this pass) of the tile
    if (tid < SP_TR) {
        const uint32_t j = j0 + tid;
        uint32_t row = 0xffffffffu;
        if (j < p.n_elig) { row = p.elig[j]; if (row >= p.n_rows) row = 0xffffffffu; }   // an entry out of range is skipped
        sRow[tid] = row;
    }
    __syncthreads();

    // staging: float4 f = tid + 256 u of a [64][32] chunk -> tile row f >> 3, 16-byte column f & 7 (8 threads = one 128-byte segment)
    const uint32_t st_r = tid >> 3, st_c = (tid & 7u) << 2;
    // sources: rows st_r, st_r + 32, queries st_r, st_r + 32.  A masked row or query reads the zero chunk instead (and does not
    // advance): no address is ever formed from an index that failed its check
    const uint32_t row_a = sRow[st_r], row_b = sRow[st_r + 32];
    const uint32_t q_a = q0 + st_r, q_b = q_a + 32;
    const bool ok0 = row_a != 0xffffffffu, ok1 = row_b != 0xffffffffu, ok2 = q_a < p.nq, ok3 = q_b < p.nq;
    const float* src0 = (ok0 ? p.rows + (size_t)row_a * p.ld : sparse_zero_chunk) + st_c;
    const float* src1 = (ok1 ? p.rows + (size_t)row_b * p.ld : sparse_zero_chunk) + st_c;
    const float* src2 = (ok2 ? p.qp + (size_t)q_a * p.ld : sparse_zero_chunk) + st_c;
    const float* src3 = (ok3 ? p.qp + (size_t)q_b * p.ld : sparse_zero_chunk) + st_c;
    const uint32_t step0 = ok0 ? KSTAGE : 0, step1 = ok1 ? KSTAGE : 0, step2 = ok2 ? KSTAGE : 0, step3 = ok3 ? KSTAGE : 0;
    const uint32_t off0 = st_r * SP_LD + st_c, off1 = off0 + 32 * SP_LD, off2 = off0 + SP_TR * SP_LD, off3 = off2 + 32 * SP_LD;
    const uint32_t n_chunks = (p.dim + KSTAGE - 1) / KSTAGE;       // (ld >= dim rounded up to KSTAGE; [dim, ld) reads as zero on both sides)
    float4 stg0 = *reinterpret_cast<const float4*>(src0);
    float4 stg1 = *reinterpret_cast<const float4*>(src1);
    float4 stg2 = *reinterpret_cast<const float4*>(src2);
    float4 stg3 = *reinterpret_cast<const float4*>(src3);
    *reinterpret_cast<float4*>(sImg + off0) = stg0;
    *reinterpret_cast<float4*>(sImg + off1) = stg1;
    *reinterpret_cast<float4*>(sImg + off2) = stg2;
    *reinterpret_cast<float4*>(sImg + off3) = stg3;
    __syncthreads();

    const uint32_t tr = lane >> 2, tq = wave * 16 + (lane & 3u) * 4;
    const bool wave_active = q0 + wave * 16 < p.nq;                // wave-uniform
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;

    for (uint32_t c = 0; c < n_chunks; ++c) {
        const bool more = c + 1 < n_chunks;
        if (more) {
            src0 += step0; src1 += step1; src2 += step2; src3 += step3;
            stg0 = *reinterpret_cast<const float4*>(src0);
            stg1 = *reinterpret_cast<const float4*>(src1);
            stg2 = *reinterpret_cast<const float4*>(src2);
            stg3 = *reinterpret_cast<const float4*>(src3);
        }
        if (wave_active) {
            const float* img = sImg + (c & 1u) * SP_IMG;
            // quads of this chunk that hold elements of the vectors (the rest is padding: +0 products, which leave the sums as they are)
            const uint32_t left = p.dim - c * KSTAGE;
            const uint32_t n_quads = left >= KSTAGE ? KSTAGE / 4 : (left + 3) / 4;
            for (uint32_t kq = 0; kq < n_quads; ++kq) {
                float4 x[4], q[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] = *reinterpret_cast<const float4*>(img + (tr + 16 * i) * SP_LD + 4 * kq);
#pragma unroll
                for (int j = 0; j < 4; ++j) q[j] = *reinterpret_cast<const float4*>(img + (SP_TR + tq + j) * SP_LD + 4 * kq);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float xv = e == 0 ? x[i].x : e == 1 ? x[i].y : e == 2 ? x[i].z : x[i].w;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const float qv = e == 0 ? q[j].x : e == 1 ? q[j].y : e == 2 ? q[j].z : q[j].w;
                            if (EUC) { const float t = __fsub_rn(qv, xv); acc[i][j] = __fadd_rn(acc[i][j], __fmul_rn(t, t)); }
                            else acc[i][j] = __fadd_rn(acc[i][j], __fmul_rn(qv, xv));
                        }
                    }
                }
            }
        }
        if (more) {
            float* nxt = sImg + ((c + 1) & 1u) * SP_IMG;           // last read in round c - 1, before that round's barrier
            *reinterpret_cast<float4*>(nxt + off0) = stg0;
            *reinterpret_cast<float4*>(nxt + off1) = stg1;
            *reinterpret_cast<float4*>(nxt + off2) = stg2;
            *reinterpret_cast<float4*>(nxt + off3) = stg3;
        }
        __syncthreads();
    }

    // ---- epilogue: distance -> key, through LDS (every read of the images is behind the loop's last barrier)
    uint64_t* sKey = reinterpret_cast<uint64_t*>(sImg);           // [SP_TQ][SP_TR]
    if (wave_active) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t row = sRow[tr + 16 * i];
            const bool row_ok = row != 0xffffffffu;
            const float xn = (row_ok && p.metric == COSINE) ? p.nd[row] : 0.0f;
            const uint32_t rk = row_ok ? (p.idrank ? p.idrank[row] : row) : 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t q = q0 + tq + j;
                uint64_t key = EMPTY_KEY;
                if (row_ok && q < p.nq) {
                    const float s = acc[i][j];
                    float dist;
                    if (EUC) dist = __builtin_sqrtf(s);
                    else if (p.metric == DOT) dist = -s;
                    else {
                        float sim = __fdiv_rn(s, __fmul_rn(p.qnorm[q], xn));   // distance.rs:58
                        if (sim < -1.0f) sim = -1.0f;                         // f32::clamp keeps NaN
                        if (sim > 1.0f) sim = 1.0f;
                        dist = __fsub_rn(1.0f, sim);
                    }
                    if (dist != dist) atomicOr(p.status, ST_NAN);
                    key = ((uint64_t)f32_to_ordered(dist) << 32) | rk;
                }
                sKey[(tq + j) * SP_TR + tr + 16 * i] = key;
            }
        }
    }
    __syncthreads();
    // keys[q * key_stride + j]: one query's 64 keys are 512 contiguous bytes.  key_stride is a multiple of SPARSE_TILE_R, so the
    // whole tile is inside the buffer; the positions past the end of the list carry EMPTY_KEY
    for (uint32_t f = tid; f < SP_TQ * SP_TR; f += 256) {
        const uint32_t ql = f / SP_TR, r = f % SP_TR;
        const uint32_t q = q0 + ql;
        if (q < p.nq && j0 + r < p.key_stride) p.keys[(size_t)q * p.key_stride + j0 + r] = sKey[f];
    }

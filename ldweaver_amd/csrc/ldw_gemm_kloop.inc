// K loop of one 128 (to side) x 64 (from side) workgroup tile of the bit-packed co-occurrence GEMM.  Textually
// included in the body of gemm_bits_kernel (ldw_gemm_bits.hip): as an inlined
// function taking the accumulators by reference the same code needs ~70 more VGPRs and spills (hipcc 7.2).
// Expects in scope: template int J; GemmSmem<J> S (shared); Mbits, KW, rowlist_t, rowlist_f, digits, Kpad; bx, by.
// Defines: tid, lane, wave, wm, wn, frow, fh and acc[J][2]: acc[j][m][e] of lane (frow, fh) of wave (wm, wn) is limb j
// of to-row by*128 + wm*64 + m*32 + (e & 3) + 8*(e >> 2) + 4*fh and from-row bx*64 + wn*32 + frow.  256 threads =
// 4 waves (2 x 2), 64 x 32 per wave = 2 MFMA tiles x J limbs.  Every wave has passed the barrier behind the last
// chunk when the loop is left, so the shared buffers may be reused.
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    // staging: to side 128 rows x 8 word pairs = 1024 pieces (4 per thread), from side 64 x 8 = 512 (2 per thread)
    const uint64_t *gT[4], *gF[2];
    int woT[4], woF[2], wpT[4], wpF[2];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int idx = tid + 256 * p;
        const int row = idx >> 3;
        wpT[p] = idx & 7;
        gT[p] = Mbits + (int64_t)rowlist_t[by * TILE + row] * KW + 2 * wpT[p];
        woT[p] = row * BROW + 2 * wpT[p];
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int idx = tid + 256 * p;
        const int row = idx >> 3;
        wpF[p] = idx & 7;
        gF[p] = Mbits + (int64_t)rowlist_f[bx * TILE_F4 + row] * KW + 2 * wpF[p];
        woF[p] = row * BROW + 2 * wpF[p];
    }
    // digits of a chunk: J*64 pieces of 16 B over 256 threads
    constexpr int DP = (J * 64 + 255) / 256;
    const int8_t *gD[DP];
    int dOfs[DP], dq[DP];
    bool dOn[DP];
#pragma unroll
    for (int p = 0; p < DP; ++p) {
        const int idx = tid + 256 * p;
        dOn[p] = idx < J * 64;
        const int dj = idx >> 6;
        dq[p] = idx & 63;
        gD[p] = digits + (int64_t)(dOn[p] ? dj : 0) * Kpad + dq[p] * 16;
        dOfs[p] = dj * (BW_CHUNK * 64) + dq[p] * 16;
    }

    v16i acc[J][2];
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[j][m][e] = 0;

    const int nchunk = (int)((KW + BW_CHUNK - 1) / BW_CHUNK);
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    u64x2 rT[4], rF[2];
    v4i rD[DP];

    auto load_chunk = [&](int c) {
        const int64_t w0 = (int64_t)c * BW_CHUNK;
        const int cw = (int)((KW - w0) < BW_CHUNK ? (KW - w0) : BW_CHUNK);
#pragma unroll
        for (int p = 0; p < 4; ++p) rT[p] = (2 * wpT[p] < cw) ? *reinterpret_cast<const u64x2 *>(gT[p] + w0) : u64x2{0ull, 0ull};
#pragma unroll
        for (int p = 0; p < 2; ++p) rF[p] = (2 * wpF[p] < cw) ? *reinterpret_cast<const u64x2 *>(gF[p] + w0) : u64x2{0ull, 0ull};
#pragma unroll
        for (int p = 0; p < DP; ++p)
            rD[p] = (dOn[p] && dq[p] * 16 < cw * 64) ? *reinterpret_cast<const v4i *>(gD[p] + w0 * 64) : v4i{0, 0, 0, 0};
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            S.sT[buf][woT[p]] = rT[p][0];
            S.sT[buf][woT[p] + 1] = rT[p][1];
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            S.sF[buf][woF[p]] = rF[p][0];
            S.sF[buf][woF[p] + 1] = rF[p][1];
        }
#pragma unroll
        for (int p = 0; p < DP; ++p)
            if (dOn[p]) *reinterpret_cast<v4i *>(&S.sD[buf][dOfs[p]]) = rD[p];
    };

    {
        const v4i lo = expand01((uint32_t)tid & 0xFFu);
        const uint64_t e01 = (uint64_t)(uint32_t)lo[0] | ((uint64_t)(uint32_t)lo[1] << 32);
        S.lut01[tid] = e01;
        S.lutFF[tid] = (e01 << 8) - e01;
    }
    load_chunk(0);
    store_chunk(0);
    __syncthreads();

    const int frow = lane & 31;
    const int fh = lane >> 5;
    const int a0o = (wm * 64 + frow) * BROW + fh, a1o = a0o + 32 * BROW, bo = (wn * 32 + frow) * BROW + fh;

    for (int c = 0; c < nchunk; ++c) {
        const int cur = c & 1;
        if (c + 1 < nchunk) load_chunk(c + 1);
        const int64_t w0 = (int64_t)c * BW_CHUNK;
        const int nmac = (int)(((KW - w0) < BW_CHUNK ? (KW - w0) : BW_CHUNK) >> 1);
        for (int m = 0; m < nmac; ++m) {
            const uint64_t a0w = S.sT[cur][a0o + 2 * m], a1w = S.sT[cur][a1o + 2 * m], bw = S.sF[cur][bo + 2 * m];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                typedef unsigned long long u64x2v __attribute__((ext_vector_type(2)));
                const u64x2v a0q = {S.lut01[(a0w >> (16 * kk)) & 0xFFu], S.lut01[(a0w >> (16 * kk + 8)) & 0xFFu]};
                const u64x2v a1q = {S.lut01[(a1w >> (16 * kk)) & 0xFFu], S.lut01[(a1w >> (16 * kk + 8)) & 0xFFu]};
                const u64x2v bq = {S.lutFF[(bw >> (16 * kk)) & 0xFFu], S.lutFF[(bw >> (16 * kk + 8)) & 0xFFu]};
                const v4i a0 = __builtin_bit_cast(v4i, a0q), a1 = __builtin_bit_cast(v4i, a1q);
                const v4i bmask = __builtin_bit_cast(v4i, bq);
                const int doff = (2 * m + fh) * 64 + kk * 16;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const v4i d = *reinterpret_cast<const v4i *>(&S.sD[cur][j * (BW_CHUNK * 64) + doff]);
                    const v4i bm = bmask & d;
                    acc[j][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, bm, acc[j][0], 0, 0, 0);
                    acc[j][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, bm, acc[j][1], 0, 0, 0);
                }
            }
        }
        if (c + 1 < nchunk) store_chunk(cur ^ 1);
        __syncthreads();
    }

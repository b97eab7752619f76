// Part of ldw_mi.hip (inside namespace ldw): the fp64 evaluation kernels — the epilogue of the plain path (every pair of a block: k_mi_epilogue_fast +
// k_mi_epilogue_rest, or the one-kernel k_mi_epilogue), k_mi_units (the units the screens list), the small utility kernels of a block's chain, the pair
// list of blocks in generic POS order (k_gen_*), k_tables / k_slot_counts (ldw_joint_tables).
// ------------------------------------------------------------------------------------------------
// The epilogue: fp64 MI of every pair of the block, emission of the pairs (dense MI block, short-range rows, LDS
// histogram / speculative candidates).  The path of blocks without a bucket guess and of ldw_mi_block.
// ------------------------------------------------------------------------------------------------
#ifndef LDW_EPI_WAVES
#define LDW_EPI_WAVES 3
#endif
#ifndef LDW_EPI_FAST_WAVES
#define LDW_EPI_FAST_WAVES 5
#endif
// columns whose joint sums k_mi_epilogue_fast requests together: 1 x 1 tables, the other variants
#ifndef LDW_EPI_U11
#define LDW_EPI_U11 4
#endif
#ifndef LDW_EPI_U
#define LDW_EPI_U 2
#endif
// ------------------------------------------------------------------------------------------------
// r06: the epilogue is TWO kernels.  k_mi_epilogue_fast takes the units whose 64 from-side SNPs all have the same 1 or 2 indicator rows,
// every slot flagged and r = their slot count, at columns of that kind (99 % of the units of C4): four straight-line variants and nothing
// else.  The units it does not take — tiles of SNPs with >= 3 minor states or unflagged slots, such columns, the columns at a class border
// of a wave's 32 — go to a LIST (tile << 32 | column slot) which k_mi_epilogue_rest walks with one wave per unit and the predicated code:
// every unit is evaluated exactly once, by the same fma chain (cells_mi_x) on the same numbers — equal joint tables give equal bits in any
// of the three kernels.  k_mi_epilogue, one kernel over the whole grid, stays as the A/B (LDW_NO_EPI_SPLIT).
// What the split buys, step by step (profiles/r06_epi_split.txt; C4, plain path, epilogue stage per pass, 60.1 ms before):
//  * registers: 89-96 instead of 156 -> 5 waves per SIMD instead of 3 (LDS histogram packed to 16-bit counters so that five workgroups fit);
//  * RM / MODE are template parameters: the kernel argument block is ~100 SGPRs of pointers and flags, and with all of them live across the
//    column loop the compiler spilled 34 of them to VGPR lanes — dozens of v_readlane per column, on the VALU the kernel is bound by;
//  * the joint sums of U columns are requested before the first is evaluated (one 512-byte request in flight per wave was latency-bound).
//    Every lane loads, whatever its pair (the addresses of a padding lane or of a pair on the wrong side of a diagonal block's diagonal lie
//    inside the block; the values are not used);
//  * the cells' pxy are formed in fp64, EXACTLY: a fixed-point sum n < 2^52 scaled by 2^-F is a double, and so is every marginal minus such
//    sums plus 1/2 (multiples of 2^-F below 2^53 units) — a derived cell costs one v_add_f64 instead of a 64-bit subtraction, a conversion
//    and an fma, and the values are bit for bit those of full_cells + pxy_of;
//  * den, rX, rY and 1 / (den / 2) depend on r alone, r is the slot-count class's: computed once per workgroup (EpiFastConst).
// ------------------------------------------------------------------------------------------------
struct EpiFastConst {
    double den, rY, hrcp, rxy0;   // for one nb (rX is the tile's); rxy0: RXY in the intended mode
};
// a fast column whose r is its slot count (the reference's r = rowSums(uqe): R/extractSNPs.R:141 — anything else goes to the list)
__device__ __forceinline__ bool col_is_fast_r(const ColMeta &M, uint32_t mb) { return col_is_fast(mb) && M.rb == (double)((int)(mb & 7) + 1); }

// MODE 0: dense block only (E.cols null: ldw_mi_block); 1: link tables, every long-range pair into the histogram; 2: link tables, speculative
// candidates (E.spec_B >= 0).  The statement of emit_pair, with the interval tests free of branches.
template <int MODE>
__device__ __forceinline__ void epi_fast_emit(const EmitArgs &E, const ColMeta &M, int a_loc, int b_loc, int sa, double mi, unsigned int *sh_hist) {
    if (E.write_dense) E.MI[(int64_t)a_loc + (int64_t)b_loc * E.nf] = mi;
    if (MODE == 0) return;
    if (a_loc == b_loc) return;   // (not a pair: quirk Q3; the lanes of a diagonal block with a_loc < b_loc never come here)
    const int seg = a_loc > b_loc ? 1 : 0;
    if (E.any_sr) {
        const ColInfo &c = M.ci;
        const bool sr = ((a_loc >= c.s[0]) & (a_loc < c.e[0])) | ((a_loc >= c.s[1]) & (a_loc < c.e[1])) | ((a_loc >= c.s[2]) & (a_loc < c.e[2]));
        if (sr) {
            if (E.keep_sr) {
                const int64_t dst = E.sr_base + (seg == 0 ? c.off_u + col_count(c, 0, a_loc) : c.off_l + col_count(c, b_loc + 1, a_loc));
                E.sr_a[dst] = sa;
                E.sr_b[dst] = M.sb;
                E.sr_mi[dst] = mi;
            }
            return;
        }
    }
    if (!E.do_lr) return;
    if (MODE == 2) {
        if (mi >= E.spec_lo) {
            const int bk = mi_bucket(mi);
            if (bk >= E.spec_B) {
                hist_bump<true>(sh_hist, bk);
                const unsigned long long p = atomicAdd(E.n_cand, 1ull);
                E.ckey[p] = f64_key(mi);
                E.cval[p] = ((uint64_t)seg << 62) | ((uint64_t)a_loc + (uint64_t)b_loc * (uint64_t)E.nf);
            }
        }
    } else {
        hist_bump<true>(sh_hist, mi_bucket(mi));
    }
}

// U columns of one straight-line variant.  RM: how RXY is read (0 intended, 1 reference quirk Q1 on a square block, 2 on a ragged one, 3 on a span)
template <int NA, int NB, int U, int RM, int MODE>
__device__ __forceinline__ void epi_fast_cols(const EpiArgs &A, const RowSide &R, const double (&pXh)[3], double rX, double qrta, int64_t ra0RF, const EpiFastConst &K,
                                              const ColMeta *cmu, int a_loc, bool a_ok, unsigned int *sh_hist) {
    int64_t raw[U][NB][NA];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        // g_entry's address with the per-lane product hoisted (ra0RF = ra0 RFpad) and the column's in scalar registers: on a diagonal block the
        // entry of a pair may only exist transposed (rows above the diagonal of ROW positions are not computed)
        const int rb0 = __builtin_amdgcn_readfirstlane(cmu[u].rb0);
        const int64_t rb0RF = (int64_t)rb0 * A.RFpad;
        int64_t off = rb0RF + R.ra0, si = 1, sj = A.RFpad;
        if (A.E.lower_only) {
            const bool tr = R.ra0 < (int64_t)rb0;
            off = tr ? ra0RF + rb0 : off;
            si = tr ? (int64_t)A.RFpad : 1;
            sj = tr ? 1 : (int64_t)A.RFpad;
        }
        const int64_t *g = A.G + off;
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int i = 0; i < NA; ++i) raw[u][j][i] = g[i * si + j * sj];
    }
    const double xs_m = -4503599627370496.0 * A.scale;   // (exact: scale is a power of two)
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const ColMeta &M = cmu[u];
        const int b_loc = M.bl;
        if (!a_ok || (A.E.lower_only && a_loc <= b_loc)) continue;
        double x[NA + 1][NB + 1], rs[NA], cs[NB], tot = 0.0;
#pragma unroll
        for (int i = 0; i < NA; ++i) rs[i] = 0.0;
#pragma unroll
        for (int j = 0; j < NB; ++j) cs[j] = 0.0;
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const double xs = fma(__longlong_as_double(raw[u][j][i] | 0x4330000000000000LL), A.scale, xs_m);   // n 2^-F
                x[i][j] = xs + 0.5;
                rs[i] += xs;
                cs[j] += xs;
                tot += xs;
            }
        double corner = pXh[NA];   // pX of the dropped state + 1/2 - sum of the column marginals + sum of the entries
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            x[NA][j] = (M.pYd[j] + 0.5) - cs[j];
            corner -= M.pYd[j];
        }
#pragma unroll
        for (int i = 0; i < NA; ++i) x[i][NB] = pXh[i] - rs[i];
        x[NA][NB] = corner + tot;
        // RXY: the values pair_rxy returns (products of small integers: exact in any order)
        double RXY;
        if (RM == 0) RXY = K.rxy0;
        else if (RM == 1) RXY = M.rq * qrta;
        else if (RM == 3) RXY = (M.rq * (double)A.rloc_t[M.ci.pad[1] + a_loc]) * 0.25;
        else {
            const uint32_t c = (uint32_t)a_loc + (uint32_t)b_loc * (uint32_t)A.nf;
            const uint32_t q = c / (uint32_t)A.nt;
            RXY = (A.r[A.idx_f[q]] * A.r[A.idx_t[c - q * (uint32_t)A.nt]]) * 0.25;
        }
#if defined(LDW_ABLATE_EPI) && LDW_ABLATE_EPI == 2   // timing ablation only (wrong results): loads and emission without the evaluation
        const double mi = (x[0][0] + x[NA][NB] + RXY) * 1e-20;
#else
        const double mi = cells_mi_x<NA, NB>(x, R.pXd, M.pYd, RXY, K.den, rX, K.rY, K.hrcp);
#endif
#if defined(LDW_ABLATE_EPI) && LDW_ABLATE_EPI == 1   // timing ablation only (wrong results): the evaluation without the emission
        if (mi == 123.456) sh_hist[threadIdx.x & 63] = 1;
#else
        epi_fast_emit<MODE>(A.E, M, a_loc, b_loc, R.sa, mi, sh_hist);
#endif
    }
}

template <int RM, int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LDW_EPI_FAST_WAVES, 8))) void k_mi_epilogue_fast(EpiArgs A, const int32_t *__restrict__ perm_f,
                                                                                                           const int32_t *__restrict__ perm_t,
                                                                                                           unsigned long long *__restrict__ ghist,
                                                                                                           uint64_t *__restrict__ rest,
                                                                                                           unsigned int *__restrict__ n_rest) {
    static_assert(64 * EPI_COLS < 65536, "16-bit histogram counters");
    __shared__ unsigned int sh_hist[NBINS / 2];   // two 16-bit counters per word (hist_bump<true>)
    __shared__ ColMeta cm[EPI_COLS];
    const bool square = A.nf == A.nt;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c_first = wave * (EPI_COLS / 4);
    const int q_base = blockIdx.y * EPI_COLS + c_first;
    int n_it = A.nt - q_base;
    n_it = n_it > EPI_COLS / 4 ? EPI_COLS / 4 : (n_it < 0 ? 0 : n_it);
    RowSide R;
    int a_loc, na0;
    const bool a_ok = load_row_side(A, perm_f, square, blockIdx.x, R, a_loc);
    unsigned int rest_cols = 0;   // this wave's columns left to k_mi_epilogue_rest
    // (the four waves of a workgroup hold the same tile: the answer is the workgroup's)
    bool tile_fast = wave_is_full(R, a_ok, na0);
    tile_fast = tile_fast && __ballot(a_ok && R.ra != (double)(na0 + 1)) == 0ull;   // (r is the slot count: EpiFastConst)
    const bool use_hist = MODE != 0 && A.E.do_lr;
    if (tile_fast) {
        double pXh[3];
        EpiFastConst K[2];
        const double rX = 0.5 * (double)(na0 + 1), qrta = R.rta * 0.25;
        const int64_t ra0RF = R.ra0 * A.RFpad;
#pragma unroll
        for (int i = 0; i < 3; ++i) pXh[i] = R.pXd[i] + 0.5;
#pragma unroll
        for (int k = 0; k < 2; ++k) {   // the same expressions as full_cells_mi's and pair_rxy's, on the class's r
            const double ra = (double)(na0 + 1), rb = (double)(k + 2);
            K[k].den = A.neff + (ra * rb) * 0.5;
            K[k].rY = 0.5 * rb;
            K[k].hrcp = fast_rcp(0.5 * K[k].den);
            K[k].rxy0 = (ra * rb) * 0.25;
        }
        if (use_hist)
            for (int i = threadIdx.x; i < NBINS / 2; i += 256) sh_hist[i] = 0;
        stage_cols(A, perm_t, square, cm);
        __syncthreads();
        for (int it = 0; it < n_it;) {
            const ColMeta *cmu = &cm[c_first + it];
            const uint32_t mb0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)cmu[0].mb);
            const int nb = (int)(mb0 & 7);
            const int U = (na0 == 1 && nb == 1) ? LDW_EPI_U11 : LDW_EPI_U;
            // the next U columns share the variant if they have the same slot count (the rule away from class borders);
            // a column that is not fast, or a group that is mixed or cut short, is left to the list
            bool same = it + U <= n_it && col_is_fast_r(cmu[0], mb0);
            for (int u = 1; same && u < U; ++u) {
                const uint32_t mbu = (uint32_t)__builtin_amdgcn_readfirstlane((int)cmu[u].mb);
                same = (int)(mbu & 7) == nb && col_is_fast_r(cmu[u], mbu);
            }
            if (!same) {
                rest_cols |= 1u << it;
                ++it;
                continue;
            }
            if (na0 == 1) {
                if (nb == 1) epi_fast_cols<1, 1, LDW_EPI_U11, RM, MODE>(A, R, pXh, rX, qrta, ra0RF, K[0], cmu, a_loc, a_ok, sh_hist);
                else epi_fast_cols<1, 2, LDW_EPI_U, RM, MODE>(A, R, pXh, rX, qrta, ra0RF, K[1], cmu, a_loc, a_ok, sh_hist);
            } else {
                if (nb == 1) epi_fast_cols<2, 1, LDW_EPI_U, RM, MODE>(A, R, pXh, rX, qrta, ra0RF, K[0], cmu, a_loc, a_ok, sh_hist);
                else epi_fast_cols<2, 2, LDW_EPI_U, RM, MODE>(A, R, pXh, rX, qrta, ra0RF, K[1], cmu, a_loc, a_ok, sh_hist);
            }
            it += U;
        }
    } else {
        rest_cols = n_it >= 32 ? 0xFFFFFFFFu : ((1u << n_it) - 1u);
    }
    if (rest_cols != 0u) {   // (wave-uniform)
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(n_rest, (unsigned int)__popc(rest_cols));
        base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
        if (lane < 32 && ((rest_cols >> lane) & 1u))
            rest[base + __popc(rest_cols & ((1u << lane) - 1u))] = ((uint64_t)blockIdx.x << 32) | (uint32_t)(q_base + lane);
    }
    if (tile_fast && use_hist) {
        __syncthreads();
        for (int i = threadIdx.x; i < NBINS / 2; i += 256) {
            const unsigned int v = sh_hist[i];
            if (v & 0xFFFFu) atomicAdd(&ghist[2 * i], (unsigned long long)(v & 0xFFFFu));
            if (v >> 16) atomicAdd(&ghist[2 * i + 1], (unsigned long long)(v >> 16));
        }
    }
}

// the units k_mi_epilogue_fast listed: one wave per unit, grid-stride, the predicated code of k_mi_epilogue
__global__ __launch_bounds__(256) void k_mi_epilogue_rest(EpiArgs A, const int32_t *__restrict__ perm_f, const int32_t *__restrict__ perm_t,
                                                          unsigned long long *__restrict__ ghist, const uint64_t *__restrict__ rest,
                                                          const unsigned int *__restrict__ n_rest) {
    __shared__ unsigned int sh_hist[NBINS];
    const unsigned int n = *n_rest;
    if ((uint64_t)blockIdx.x * 4u * ((n + gridDim.x * 4u - 1u) / (gridDim.x * 4u)) >= n) return;   // (no entry for any wave of this workgroup)
    const bool use_hist = A.E.cols && A.E.do_lr;
    if (use_hist) {
        for (int i = threadIdx.x; i < NBINS; i += 256) sh_hist[i] = 0;
        __syncthreads();
    }
    const bool square = A.nf == A.nt;
    int cur_tile = -1, a_loc = 0, na0 = 0, na_max = 1;
    bool a_ok = false, wave_full = false;
    RowSide R;
    // (consecutive entries per wave: a wave of the fast kernel lists its columns of one tile in one run — see k_mi_units)
    const unsigned int nwaves = gridDim.x * 4u, per = (n + nwaves - 1u) / nwaves;
    const unsigned int i_begin = (blockIdx.x * 4u + (threadIdx.x >> 6)) * per, i_end = i_begin + per < n ? i_begin + per : n;
    for (unsigned int i = i_begin; i < i_end; ++i) {
        const uint64_t u = rest[i];
        const int tile = __builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32)), q = __builtin_amdgcn_readfirstlane((int)(uint32_t)u);
        if (tile != cur_tile) {
            a_ok = load_row_side(A, perm_f, square, tile, R, a_loc);
            na_max = (__ballot(R.na > 2) != 0ull) ? 4 : ((__ballot(R.na > 1) != 0ull) ? 2 : 1);
            wave_full = wave_is_full(R, a_ok, na0);
            cur_tile = tile;
        }
        ColMeta M;
        load_col(A, perm_t, square, q, M);
        const uint32_t mbu = (uint32_t)__builtin_amdgcn_readfirstlane((int)M.mb);
        const int b_loc = M.bl;
        if (!a_ok) continue;
        if (A.E.lower_only && a_loc <= b_loc) continue;
        const double mi = unit_pair_mi(A, R, M, a_loc, b_loc, square, wave_full && col_is_fast(mbu), na0, na_max, (int)(mbu & 7), g_entry(A, R, M));
        emit_pair(A.E, M.ci, a_loc, b_loc, R.sa, M.sb, mi, sh_hist);
    }
    if (use_hist) {
        __syncthreads();
        for (int i = threadIdx.x; i < NBINS; i += 256)
            if (sh_hist[i]) atomicAdd(&ghist[i], (unsigned long long)sh_hist[i]);
    }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LDW_EPI_WAVES, 8))) void k_mi_epilogue(EpiArgs A, const int32_t *__restrict__ perm_f, const int32_t *__restrict__ perm_t,
                                                     unsigned long long *__restrict__ ghist) {
    __shared__ unsigned int sh_hist[NBINS];
    __shared__ ColMeta cm[EPI_COLS];
    const bool use_hist = A.E.cols && A.E.do_lr;
    if (use_hist)
        for (int i = threadIdx.x; i < NBINS; i += 256) sh_hist[i] = 0;
    const bool square = A.nf == A.nt;
    stage_cols(A, perm_t, square, cm);
    __syncthreads();

    // lanes walk the from-side SNPs in an order that groups equal slot counts, so that a wave runs the same cells
    const int wave = threadIdx.x >> 6;
    RowSide R;
    int a_loc, na0;
    const bool a_ok = load_row_side(A, perm_f, square, blockIdx.x, R, a_loc);
    const int na_max = (__ballot(R.na > 2) != 0ull) ? 4 : ((__ballot(R.na > 1) != 0ull) ? 2 : 1);
    const bool wave_full = wave_is_full(R, a_ok, na0);

    const int c_first = wave * (EPI_COLS / 4);
    const int q_base = blockIdx.y * EPI_COLS + c_first;
    int n_it = A.nt - q_base;
    n_it = n_it > EPI_COLS / 4 ? EPI_COLS / 4 : n_it;
    for (int it = 0; it < n_it; ++it) {
        const ColMeta &M = cm[c_first + it];
        const uint32_t mbu = (uint32_t)__builtin_amdgcn_readfirstlane((int)M.mb);
        const int b_loc = M.bl;
        if (!a_ok) continue;
        if (A.E.lower_only && a_loc <= b_loc) continue;
        const double mi = unit_pair_mi(A, R, M, a_loc, b_loc, square, wave_full && col_is_fast(mbu), na0, na_max, (int)(mbu & 7), g_entry(A, R, M));
        emit_pair(A.E, M.ci, a_loc, b_loc, R.sa, M.sb, mi, sh_hist);
    }
    if (use_hist) {
        __syncthreads();
        for (int i = threadIdx.x; i < NBINS; i += 256)
            if (sh_hist[i]) atomicAdd(&ghist[i], (unsigned long long)sh_hist[i]);
    }
}

// ------------------------------------------------------------------------------------------------
// k_mi_units: the fp64 evaluation of the units listed by k_mi_screen (speculative selection mode): one wave per unit,
// grid-stride over the list.  A few per cent of the block's units are listed, so what counts is latency (the SNP
// constants of both sides are fetched per unit) — hidden by the number of waves in flight — not throughput.
// ------------------------------------------------------------------------------------------------
// FAST: list 0, straight-line variants only — half the registers of the predicated code, so that its waves fit on a CU beside
// the two workgroups of the next block's GEMM (which runs on the other stream) instead of waiting for them to drain.
// Where a launch of k_mi_units finds its units: up to 4 flat lists (blockIdx.y)
struct UnitLists {
    const uint64_t *units[4];
    const unsigned int *n[4];
};

__device__ unsigned long long g_viol_n;
__device__ double g_viol_rec[64];

template <bool FAST>
__global__ __launch_bounds__(256) void k_mi_units(EpiArgs A, const int32_t *__restrict__ perm_f, const int32_t *__restrict__ perm_t,
                                                  UnitLists UL, unsigned long long *__restrict__ ghist) {
    const bool square = A.nf == A.nt;
    const int y = blockIdx.y;
    const uint64_t *__restrict__ units = UL.units[y];
    const unsigned int n = *UL.n[y];
    // a wave takes CONSECUTIVE entries: a screen wave appends its units — one tile, up to 32 columns — in one run, so the per-lane constants of
    // the tile (200 bytes per lane) are fetched once per run, not once per unit (r06: with a grid-strided walk every unit changed the tile)
    const unsigned int nwaves = gridDim.x * 4u, per = (n + nwaves - 1u) / nwaves;
    const unsigned int i_begin = (blockIdx.x * 4u + (threadIdx.x >> 6)) * per, i_end = i_begin + per < n ? i_begin + per : n;
    int cur_tile = -1, a_loc = 0, na0 = 0, na_max = 1;
    bool a_ok = false, wave_full = false;
    RowSide R;
    for (unsigned int i = i_begin; i < i_end; ++i) {
        const uint64_t u = units[i];
        const uint32_t ulo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u);
        const uint32_t uhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
        const bool dismissed = (uhi & 0x80000000u) != 0;
        const uint32_t v = ulo & 0x7FFFFFFFu;
        const int tile = (int)(v / (uint32_t)A.nt), q = (int)(v - (uint32_t)tile * (uint32_t)A.nt);
        if (tile != cur_tile) {
            a_ok = load_row_side(A, perm_f, square, tile, R, a_loc);
            na_max = (__ballot(R.na > 2) != 0ull) ? 4 : ((__ballot(R.na > 1) != 0ull) ? 2 : 1);
            wave_full = wave_is_full(R, a_ok, na0);
            cur_tile = tile;
        }
        ColMeta M;
        load_col(A, perm_t, square, q, M);
        const uint32_t mbu = (uint32_t)__builtin_amdgcn_readfirstlane((int)M.mb);
        const int b_loc = M.bl;
        if (!a_ok) continue;
        if (A.E.lower_only && a_loc <= b_loc) continue;
        GAcc Ga = g_entry(A, R, M);
        if (A.lo.on) {   // G holds the high limbs only: the low limbs of this unit's joint sums come from the gathered GEMM
            const int k = (int)(((ulo >> 31) | (uhi << 1)) & 0xFFFFFu), lc = (int)((uhi >> 19) & 3u);
            const int cmax = A.lo.cmax_f[tile];
            const int64_t ld = 64 * (int64_t)cmax;
            Ga.l = A.lo.glo + A.lo.tile_base[tile] + ((int64_t)A.lo.rowbase[lc] + ((int64_t)k << lc)) * ld + (int64_t)(threadIdx.x & 63) * cmax;
            Ga.li = 1;
            Ga.lj = ld;
            Ga.shift = A.lo.hi_shift;
        }
        double mi;
        if (FAST) {
            const int nb = (int)(mbu & 7);
            if (na0 == 1) mi = nb == 1 ? pair_mi_full<1, 1>(A, R, M, a_loc, b_loc, square, Ga) : pair_mi_full<1, 2>(A, R, M, a_loc, b_loc, square, Ga);
            else mi = nb == 1 ? pair_mi_full<2, 1>(A, R, M, a_loc, b_loc, square, Ga) : pair_mi_full<2, 2>(A, R, M, a_loc, b_loc, square, Ga);
        } else {
            mi = unit_pair_mi(A, R, M, a_loc, b_loc, square, wave_full && col_is_fast(mbu), na0, na_max, (int)(mbu & 7), Ga);
        }
        if (dismissed) {   // verify mode: a pair of a dismissed unit that would have been emitted was lost by the screen
            if (would_emit(A.E, M.ci, a_loc, b_loc, mi)) {
                atomicAdd(A.E.scr_viol, 1ull);
                const unsigned long long k = atomicAdd(&g_viol_n, 1ull);   // inspection only: the first violations of the process (ldw_debug_violations)
                if (k < 16) {
                    g_viol_rec[k * 4 + 0] = (double)R.sa;
                    g_viol_rec[k * 4 + 1] = (double)M.sb;
                    g_viol_rec[k * 4 + 2] = mi;
                    g_viol_rec[k * 4 + 3] = (double)A.E.spec_lo;
                }
            }
            continue;
        }
        emit_pair_spec(A.E, M.ci, a_loc, b_loc, R.sa, M.sb, mi, ghist);
    }
}

// one launch instead of four or five hipMemsetAsync per block (each a 4-5 us kernel of its own plus a dispatch gap): zeroes up to
// four small buffers, sizes in 16-byte pieces
struct ZeroArgs {
    uint4 *p[6];
    unsigned int n16[6];
};
__global__ __launch_bounds__(256) void k_zero4(ZeroArgs Z) {
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int k = 0; k < 6; ++k)
        for (unsigned int i = blockIdx.x * 256u + threadIdx.x; i < Z.n16[k]; i += gridDim.x * 256u) Z.p[k][i] = z;
}

// totals of the approximate path's lists (diagnostics: ldw_ctx_counters2): units listed (they hold a short-range pair),
// long-range candidate pairs listed
__global__ void k_apx_stats(const unsigned int *__restrict__ n_units, const unsigned int *__restrict__ pl_n, unsigned int pl_cap,
                            unsigned long long *__restrict__ acc) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    acc[0] += (unsigned long long)n_units[0] + n_units[1];
    unsigned long long k = 0;
    if (pl_n)
        for (int i = 0; i < PAIR_PATHS * PAIR_SHARDS; ++i) k += pl_n[i] > pl_cap ? pl_cap : pl_n[i];
    acc[1] += k;
    if (pl_n) acc[2] += (unsigned long long)pl_n[PH_MAYBE_N];   // r05: entries the GEMM's epilogue handed to the maybe list (0 when the list is off)
}

// ------------------------------------------------------------------------------------------------
// Blocks whose SNP lists are NOT ascending in POS (the reference imposes no order on snp.dat$POS: R/computePairwiseMI.R:176-177,
// :306-333 work on whatever order the lists have).  The short-range partners of a column are then no index interval, so the
// interval machinery (ColInfo, the band masks, the screens) does not apply: such a block runs the plain path — exact GEMM + fp64 MI
// of every pair into the dense block — and these three kernels do the reference's pair list on it with the predicate itself
// (len = circ_len(pos1, pos2) <= sr_dist per pair): counts per column, short-range rows to their final place (all upper rows
// column-major, then all lower rows: R/computePairwiseMI.R:306-310), long-range histogram and candidate gather.  One wave per column.
// ------------------------------------------------------------------------------------------------
struct GenArgs {
    const double *MI;            // dense block, column-major nf x nt
    int nf, nt, lower_only, keep_sr, do_lr;
    const int32_t *idx_f, *idx_t, *POS;
    double g, sr_dist;
};

__device__ __forceinline__ bool gen_is_sr(const GenArgs &S, int a_loc, double pos1) {
    return circ_len(pos1, (double)S.POS[S.idx_f[a_loc]], S.g) <= S.sr_dist;
}

__global__ __launch_bounds__(256) void k_gen_count(GenArgs S, int32_t *__restrict__ cnt_u, int32_t *__restrict__ cnt_l,
                                                   unsigned long long *__restrict__ ghist) {
    __shared__ unsigned int sh_hist[NBINS];
    for (int i = threadIdx.x; i < NBINS; i += 256) sh_hist[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, b_loc = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b_loc < S.nt) {
        const double pos1 = (double)S.POS[S.idx_t[b_loc]];
        const double *col = S.MI + (int64_t)b_loc * S.nf;
        int cu = 0, cl = 0;
        for (int a_loc = lane; a_loc < S.nf; a_loc += 64) {
            const int seg = pair_seg(a_loc, b_loc, S.lower_only);
            if (seg < 0) continue;
            if (gen_is_sr(S, a_loc, pos1)) {
                cu += seg == 0;
                cl += seg == 1;
            } else if (S.do_lr) {
                atomicAdd(&sh_hist[mi_bucket(col[a_loc])], 1u);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            cu += __shfl_xor(cu, off);
            cl += __shfl_xor(cl, off);
        }
        if (lane == 0) {
            cnt_u[b_loc] = cu;
            cnt_l[b_loc] = cl;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NBINS; i += 256)
        if (sh_hist[i]) atomicAdd(&ghist[i], (unsigned long long)sh_hist[i]);
}

// off_u / off_l: first row of the column's upper / lower short-range rows, relative to sr_base
__global__ __launch_bounds__(256) void k_gen_emit_sr(GenArgs S, const int64_t *__restrict__ off_u, const int64_t *__restrict__ off_l, int64_t sr_base,
                                                     int32_t *__restrict__ sr_a, int32_t *__restrict__ sr_b, double *__restrict__ sr_mi) {
    const int lane = threadIdx.x & 63, b_loc = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b_loc >= S.nt) return;
    const int sb = S.idx_t[b_loc];
    const double pos1 = (double)S.POS[sb];
    const double *col = S.MI + (int64_t)b_loc * S.nf;
    int64_t ru = sr_base + off_u[b_loc], rl = sr_base + off_l[b_loc];
    for (int a0 = 0; a0 < S.nf; a0 += 64) {
        const int a_loc = a0 + lane;
        int seg = -1;
        bool sr = false;
        if (a_loc < S.nf) {
            seg = pair_seg(a_loc, b_loc, S.lower_only);
            sr = seg >= 0 && gen_is_sr(S, a_loc, pos1);
        }
        const unsigned long long mu = __ballot(sr && seg == 0), ml = __ballot(sr && seg == 1);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (sr) {
            const int64_t dst = seg == 0 ? ru + __popcll(mu & below) : rl + __popcll(ml & below);
            sr_a[dst] = S.idx_f[a_loc];
            sr_b[dst] = sb;
            sr_mi[dst] = col[a_loc];
        }
        ru += __popcll(mu);
        rl += __popcll(ml);
    }
}

// ------------------------------------------------------------------------------------------------
// joint tables for explicit pairs (test / inspection API): table[p][X][Y] from G entry (p, p)
// ------------------------------------------------------------------------------------------------
__global__ void k_tables(const int64_t *__restrict__ G, int RFpad, const int32_t *idx_f, const int32_t *lrow_f,
                         const int32_t *idx_t, const int32_t *lrow_t, int np, const uint32_t *slot_meta,
                         const int64_t *marg /* [L][5] by slot */, int64_t *out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const int sa = idx_f[p], sb = idx_t[p];
    const uint32_t ma = slot_meta[sa], mb = slot_meta[sb];
    const int na = ma & 7, nb = mb & 7;
    int64_t cell[5][5];
    for (int i = 0; i <= 4; ++i)
        for (int j = 0; j <= 4; ++j) cell[i][j] = 0;
    int64_t rs[5] = {0, 0, 0, 0, 0}, cs[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) {
            const int64_t v = G[((int64_t)lrow_t[p] + j) * RFpad + lrow_f[p] + i];
            cell[i][j] = v;
            rs[i] += v;
            cs[j] += v;
        }
    int64_t dd = marg[(int64_t)sa * 5 + na];
    for (int i = 0; i < na; ++i) cell[i][nb] = marg[(int64_t)sa * 5 + i] - rs[i];
    for (int j = 0; j < nb; ++j) {
        cell[na][j] = marg[(int64_t)sb * 5 + j] - cs[j];
        dd -= cell[na][j];
    }
    cell[na][nb] = dd;
    int64_t *o = out + (int64_t)p * 25;
    for (int k = 0; k < 25; ++k) o[k] = 0;
    for (int i = 0; i <= na; ++i)
        for (int j = 0; j <= nb; ++j) {
            const int X = (ma >> (8 + 3 * i)) & 7, Y = (mb >> (8 + 3 * j)) & 7;
            o[X * 5 + Y] = cell[i][j];
        }
}

// unit-weight marginals by slot = state counts reordered
__global__ void k_slot_counts(const int32_t *counts, const uint32_t *slot_meta, int64_t L, int64_t *out) {
    const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (a >= L) return;
    const uint32_t m = slot_meta[a];
    const int n = m & 7;
    for (int i = 0; i < 5; ++i) out[a * 5 + i] = (i <= n) ? counts[a * 5 + ((m >> (8 + 3 * i)) & 7)] : 0;
}


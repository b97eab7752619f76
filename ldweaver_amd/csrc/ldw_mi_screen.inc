// Part of ldw_mi.hip (one translation unit, inside namespace ldw): per-block SNP constants (k_build_packs), the fp32 screens of the speculative
// blocks (k_mi_screen, k_mi_screen_generic, k_screen_maybe), the threshold table of the biallelic pairs (k_build_tab11) and the exact per-pair MI
// entry points they share with the evaluation kernels.  See the header comment of ldw_mi.hip for how the kernels chain.

// the exact-sum block of pipeline slot s
static inline ldw::DevBuf &gx(ldw_ctx *c, int s) { return s == 0 ? c->G : (s == 1 ? c->G2 : c->G3); }

// Per-block SNP constants in epilogue order, once per block instead of once per workgroup (k_mi_screen) or per unit
// (k_mi_units): blockIdx.y = 0: thread i builds column slot i (i < nt); blockIdx.y = 1: from-side slot i (i < 64 * tiles) — two independent chains
// of dependent loads, side by side instead of one after the other in the same thread (24 -> 13 us per C4 block); A.colpack / A.rowpack are null here.
__global__ __launch_bounds__(256) void k_build_packs(EpiArgs A, const int32_t *__restrict__ perm_f, const int32_t *__restrict__ perm_t,
                                                     int nf_slots, int with_hi, ColMeta *__restrict__ cp, ColMeta *__restrict__ cp_hi,
                                                     RowPack *__restrict__ rp, RowPack *__restrict__ rp_hi, float *__restrict__ rloc_f,
                                                     float *__restrict__ rloc_t, uint8_t *__restrict__ bin_t = nullptr,
                                                     uint8_t *__restrict__ bin_f = nullptr, int RTpad = 0, int RFpad = 0,
                                                     uint8_t *__restrict__ sflag_f = nullptr, uint8_t *__restrict__ sflag_t = nullptr,
                                                     uint8_t *__restrict__ rflag_f = nullptr, uint8_t *__restrict__ rflag_t = nullptr,
                                                     MiniCol *__restrict__ mini_c = nullptr, MiniRow *__restrict__ mini_r = nullptr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool square = A.nf == A.nt;
    // pruning flags (PF_*): kind of the SNP and whether its bound (k_snp_sup) stays below the block's level for partners of kind 2 / 3;
    // by epilogue slot for the screen, by row of the row lists (zeroed beforehand: padding rows) for the approximate GEMM
    const double lvl = A.E.spec_lo - (double)A.E.scr_eps;
    auto prune_flags = [&](int snp, uint32_t meta, double r) -> unsigned {
        const int n = (int)(meta & 7);
        const uint32_t full = (2u << n) - 1u;
        if (!(n == 1 || n == 2) || ((meta >> 3) & full) != full || r != (double)(n + 1)) return 0u;
        const double *sp = A.snp_sup + (int64_t)snp * 4 + (A.quirk == LDW_QUIRK_REFERENCE ? 2 : 0);
        return (unsigned)(n + 1) | (sp[0] < lvl ? PF_DEAD2 : 0u) | (sp[1] < lvl ? PF_DEAD3 : 0u);
    };
    // bins of the threshold table by ROW of the two row lists for the GEMM's epilogue test (only used when the host has checked
    // that a one-row SNP's position in its row list equals its slot here: no SNP without a row in the block)
    int my_bt = 255, my_bf = 255;
    const bool to_side = blockIdx.y == 0;
    if (!to_side && i < A.nf) rloc_f[i] = (float)A.r[A.idx_f[i]];
    if (to_side && i < A.nt) rloc_t[i] = (float)A.r[A.idx_t[i]];
    if (to_side && i < A.nt) {
        ColMeta m;
        load_col(A, perm_t, square, i, m, false);
        if (A.span) {   // a column of a span: its index within ITS reference block, and the r of quirk Q1 on that (square) block
            m.bl -= m.ci.pad[1];
            m.rq = A.r[A.idx_f[m.bl]];
        }
        cp[i] = m;
        if ((m.mb & 7) == 1 && col_is_fast(m.mb) && m.rb == 2.0) my_bt = m.pad2 & 63;
        if (sflag_t) {
            const unsigned f = prune_flags(m.sb, m.mb, m.rb);
            sflag_t[i] = (uint8_t)f;
            for (int j = 0; j < (int)(m.mb & 7); ++j) rflag_t[m.rb0 + j] = (uint8_t)f;
        }
        if (with_hi) {
#pragma unroll
            for (int j = 0; j < 5; ++j) m.pb[j] = A.lo.slot_pfix_hi[(int64_t)m.sb * 5 + j];
            cp_hi[i] = m;
            if (mini_c) mini_c[i] = MiniCol{(int32_t)m.pb[0], m.pYf[0], m.pYf[1], (float)m.rb, (float)m.rq, m.bl, m.ci.pad[1], m.sb};
        }
    }
    if (!to_side && i < nf_slots) {
        RowPack P;
        int a_loc;
        const bool ok = load_row_side_at(A, perm_f, square, i, P.R, a_loc, false);
        P.a_loc = ok ? a_loc : -1;
        P.pad = A.tab11 ? tab_bin(P.R.pXf[0], A.tab_c, A.tab_nb) : 0;   // bin of the minor-state marginal (threshold table)
        rp[i] = P;
        if (ok && P.R.na == 1 && ((P.R.ma >> 3) & 3u) == 3u && P.R.ra == 2.0) my_bf = P.pad & 63;
        if (sflag_f) {
            const unsigned f = ok ? prune_flags(P.R.sa, P.R.ma, P.R.ra) : PF_PAD;
            sflag_f[i] = (uint8_t)f;
            if (ok)
                for (int j = 0; j < P.R.na; ++j) rflag_f[P.R.ra0 + j] = (uint8_t)f;
        }
        if (with_hi) {
#pragma unroll
            for (int k = 0; k < 5; ++k) P.R.pa[k] = A.lo.slot_pfix_hi[(int64_t)P.R.sa * 5 + k];
            rp_hi[i] = P;
            if (mini_r) mini_r[i] = MiniRow{(int32_t)P.R.pa[0], (int32_t)P.R.pa[1], P.R.pXf[0], P.R.pXf[1], (float)P.R.ra, (float)P.R.rta, P.a_loc, P.R.sa};
        }
    }
    if (to_side && bin_t && i < RTpad) bin_t[i] = (uint8_t)my_bt;
    if (!to_side && bin_f && i < RFpad) bin_f[i] = (uint8_t)my_bf;
}

// ------------------------------------------------------------------------------------------------
// k_mi_screen: the fp32 screen of the two-kernel path (speculative selection mode).  A long-range pair only matters if
// its MI reaches the guessed histogram bucket, which about one pair in a thousand does; this kernel bounds MI in fp32
// (full_cells_screen, ldw_epi.h) for every unit whose SNPs have 1 or 2 fully flagged slots and writes ONE byte per
// unit: does any of its 64 pairs need the exact value (short-range pair, or upper bound >= the bucket's lower edge)?
// k_mi_epilogue then evaluates only the flagged units (and the units this kernel does not handle).  The kernel is kept
// free of the fp64 path on purpose: ~70 VGPRs instead of 145, so 6-7 waves per SIMD hide the latency of the G loads
// that bound the one-kernel epilogue (one 512-B load in flight per wave, 3 waves per SIMD: 1.3 TB/s), and U columns per
// iteration put U independent loads in flight per wave.
// ------------------------------------------------------------------------------------------------
// long-range candidates of a wave -> pair lists (approximate-GEMM path).  r06: DEFERRED — a lane only marks the column (bit = its index among the
// wave's columns) in the mask of the column's shape; the wave appends everything it found ONCE, behind its last column (flush_pairs: one atomic per
// list).  Appending at the column — an atomic whose return the whole wave waited for, four dependent look-ups of the bit rows, in the middle of the
// column loop, for ~3 % of the (wave, column) groups — cost 215 of a span screen's 696 us (ablation: profiles/r06_screen_appends.txt).
struct PendPairs {
    unsigned int m[2];   // columns with 1 / 2 indicator rows (k_mi_screen: the tile's row count is the wave's) — or [0] alone (k_mi_screen_generic)
    int q_base;          // column slot of bit 0
};
__device__ __forceinline__ void mark_pair(PendPairs &pp, int which, bool mine, int q) {
    if (mine) pp.m[which] |= 1u << (q - pp.q_base);
}
// cmw: the wave's columns in LDS (entry c = column slot q_base + c); sa: the lane's from-side SNP
__device__ __forceinline__ void flush_pairs(const EpiArgs &A, int path, unsigned int mask, int q_base, int tile, int sa, const ColMeta *cmw) {
    const int lane = threadIdx.x & 63;
    const unsigned int cnt = (unsigned int)__popc(mask);
    if (__ballot(cnt != 0u) == 0ull) return;
    unsigned int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    const unsigned int tot = (unsigned int)__builtin_amdgcn_readlane((int)incl, 63);
    const int sub = path * PAIR_SHARDS + (tile & (PAIR_SHARDS - 1));   // (sharded by tile)
    unsigned int base = 0;
    if (lane == 0) base = atomicAdd(A.pl_n + sub, tot);
    base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
    if (cnt != 0u) {
        unsigned int pos = base + incl - cnt;
        const int32_t r0a = A.row0[sa];
        const uint32_t era = (uint32_t)r0a | ((uint32_t)(A.row0[sa + 1] - r0a) << 29);
        for (unsigned int mk = mask; mk != 0u; mk &= mk - 1u, ++pos) {
            if (pos >= A.pl_cap) continue;   // overflow: k_pick_bucket sees the counter
            const int c = __builtin_ctz(mk);
            const int sb = cmw[c].sb;
            const int32_t r0b = A.row0[sb];
            PairEnt e;
            e.t = (uint32_t)(tile * 64 + lane);
            e.q = (uint32_t)(q_base + c);
            e.ra = era;
            e.rb = (uint32_t)r0b | ((uint32_t)(A.row0[sb + 1] - r0b) << 29);
            A.pl_pairs[(int64_t)sub * A.pl_cap + pos] = e;
        }
    }
}

template <int NA, int NB, int U, int RM, bool APX>
__device__ __forceinline__ unsigned int screen_cols(const EpiArgs &A, const RowSide &R, const ColMeta *cmu, int a_loc, bool a_ok, float lo, int q0, int tile, PendPairs &pp) {
    const bool test_sr = A.E.any_sr != 0 || A.sr_excl != 0, keep_sr = A.E.keep_sr != 0 && !A.sr_excl, do_lr = A.E.do_lr != 0;
    FullCells<NA, NB> C[U];
    if (do_lr) {   // an SR-only pass needs no MI here at all: a unit is wanted iff it holds a short-range pair
#pragma unroll
        for (int u = 0; u < U; ++u) full_cells<NA, NB>(R, cmu[u], g_entry(A, R, cmu[u]), C[u]);
    }
    unsigned int bits = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const ColMeta &M = cmu[u];
        const int b_loc = M.bl;
        const bool act = a_ok && (A.E.lower_only ? a_loc > b_loc : a_loc != b_loc);
        float ms = 0.0f;
        if (do_lr) ms = full_cells_screen<NA, NB, APX>(A, R, M, screen_rxy(A, R, M, a_loc, b_loc, RM), C[u]);
        const bool is_sr = test_sr && col_is_sr(M.ci, a_loc);
        if (APX && A.pl_pairs) {
            // a unit with a short-range pair is evaluated whole (its band is dense); otherwise only the candidates themselves
            const bool need_lr = act && !is_sr && do_lr && ms >= lo;
            if (__ballot(act && is_sr && keep_sr) != 0ull) bits |= 1u << u;
            else mark_pair(pp, NB - 1, need_lr, q0 + u);
        } else {
            const bool need = act && (is_sr ? keep_sr : (do_lr && ms >= lo));
            if (__ballot(need) != 0ull) bits |= 1u << u;
        }
    }
    return bits;
}

#ifdef LDW_SCREEN_STATS
__device__ unsigned long long g_scr_stats[16];
#endif
// r04: the same columns on the approximate path with pair lists, for blocks whose entries are never read transposed (all but the diagonal
// ones).  Measured (LDW_SCREEN_EXP, profiles/r04_screen_breakdown.txt): 73 % of a span's screen is this multi-cell evaluation, and its waves
// spend 73 % of their cycles waiting (SQ_WAIT_ANY / SQ_WAVE_CYCLES) with the VALU at 45 %: two columns' entries in flight per wave were too
// few.  Here the entries of all U columns (and the r look-ups of quirk Q1 on a span) are requested up front — to-side row base in SGPRs, the
// lane's from-side row as a 32-bit offset — and the tables are built in int32 from registers, one column at a time.
template <int NA, int NB, int U, int RM>
__device__ __forceinline__ unsigned int screen_cols_apx(const EpiArgs &A, const RowSide &R, const ColMeta *cmu, int a_loc, bool a_ok, float lo, int q0,
                                                        int tile, PendPairs &pp) {
    const bool test_sr = A.E.any_sr != 0 || A.sr_excl != 0, keep_sr = A.E.keep_sr != 0 && !A.sr_excl, do_lr = A.E.do_lr != 0;
    const int32_t *G32 = reinterpret_cast<const int32_t *>(A.G);
    int raw[U][NB][NA];
    float rl[U];
    if (do_lr) {   // (an SR-only pass needs no MI here at all: a unit is wanted iff it holds a short-range pair)
        if (!A.E.lower_only) {
            const uint32_t ra0 = (uint32_t)R.ra0;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int rb0 = __builtin_amdgcn_readfirstlane(cmu[u].rb0);
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    const int32_t *row = G32 + (int64_t)(rb0 + j) * A.RFpad;
#pragma unroll
                    for (int i = 0; i < NA; ++i) raw[u][j][i] = row[ra0 + (uint32_t)i];
                }
            }
        } else {
            // a diagonal block: the GEMM skips the tiles above the diagonal of ROW positions, so the entry of a pair may only exist transposed
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t rb0 = cmu[u].rb0;
                const bool tr = R.ra0 < rb0;
                const int32_t *g = G32 + (tr ? R.ra0 * A.RFpad + rb0 : rb0 * A.RFpad + R.ra0);
                const int64_t si = tr ? (int64_t)A.RFpad : 1, sj = tr ? 1 : (int64_t)A.RFpad;
#pragma unroll
                for (int j = 0; j < NB; ++j)
#pragma unroll
                    for (int i = 0; i < NA; ++i) raw[u][j][i] = g[i * si + j * sj];
            }
        }
        if (RM == 3) {
#pragma unroll
            for (int u = 0; u < U; ++u) rl[u] = A.rloc_t[__builtin_amdgcn_readfirstlane(cmu[u].ci.pad[1]) + (a_loc < 0 ? 0 : a_loc)];
        }
    }
    unsigned int bits = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const ColMeta &M = cmu[u];
        const int b_loc = M.bl;
        float ms = 0.0f;
        if (do_lr) {
            FullCells32<NA, NB> C;
            full_cells32<NA, NB>(R, M, raw[u], C);
            // (r is a small integer: the products are exact in fp32, the value is the one screen_rxy returns)
            const float rxy = RM == 3 ? ((float)M.rq * rl[u]) * 0.25f : (float)screen_rxy(A, R, M, a_loc, b_loc, RM);
#ifdef LDW_ABLATE_SCREEN_MATH   // timing ablation only (wrong results): the loads and the control flow without the bound's arithmetic
            ms = (float)(C.n[NA][NB] ^ C.n[0][0]) * 1e-30f + rxy * 1e-30f;
#else
            ms = full_cells_screen<NA, NB, true>(A, R, M, (double)rxy, C);
#endif
#ifdef LDW_SCREEN_STATS   // measurement build only: how often would a cheaper first-level bound let a pair / a (wave, column) through?
            {
                const float ra = (float)R.ra, rb = (float)M.rb, den = (float)A.neff + (ra * rb) * 0.5f, Lden = __builtin_amdgcn_logf(den);
                float S = 0.0f, SA = 0.0f, xs = 0.0f, SC = 0.0f;
#pragma unroll
                for (int i = 0; i <= NA; ++i)
#pragma unroll
                    for (int j = 0; j <= NB; ++j) {
                        const int nn = C.n[i][j];
                        const float x = fmaf((float)(nn < 0 ? 0 : nn), A.E.scr_scale, 0.5f);
                        const float dl = (R.pXf[i] + 1.0f) * (M.pYf[j] + 1.0f);
                        const float l = __builtin_amdgcn_logf(x) + Lden - __builtin_amdgcn_logf(dl);
                        S = fmaf(x, l, S);
                        SA = fmaf(x, fabsf(l), SA);
                        xs += x;
                        SC += x * x * den * __builtin_amdgcn_rcpf(dl) - x;
                    }
                const float EG = A.E.apx_EG, MU = A.E.apx_MU;
                const float lost_units = (float)(NA * NB) * EG + (float)NA * fmaxf(MU, (float)NB * EG) + (float)NB * fmaxf(MU, (float)NA * EG) +
                                         fmaxf((float)NB * MU, MU + (float)(NA * NB) * EG);
                int64_t ta = 0;
#pragma unroll
                for (int i = 0; i <= NA; ++i) ta += R.pa[i];
                const float dW = (float)(A.E.apx_W - (double)ta * A.E.apx_unit) + 4e-6f * (float)A.E.apx_W;
                const float ex = A.E.apx_dfac * fmaf(SA + 2.65f * xs, 0.6931471805599453f, A.E.apx_c1 * xs) + lost_units * A.E.apx_s1 + dW;
                const float U1 = fmaf(S, 0.6931471805599453f, ex) * __builtin_amdgcn_rcpf(den), U2 = (SC + ex) * __builtin_amdgcn_rcpf(den);
                const bool actl = a_ok && a_loc != M.bl;
                const unsigned long long b0 = __ballot(actl), b1 = __ballot(actl && ms >= lo), b2 = __ballot(actl && U1 >= lo), b3 = __ballot(actl && U2 >= lo),
                                         v1 = __ballot(actl && U1 < ms), v2 = __ballot(actl && U2 < ms);
                if ((threadIdx.x & 63) == 0) {
                    atomicAdd(&g_scr_stats[0], (unsigned long long)__popcll(b0));
                    atomicAdd(&g_scr_stats[1], (unsigned long long)__popcll(b1));
                    atomicAdd(&g_scr_stats[2], (unsigned long long)__popcll(b2));
                    atomicAdd(&g_scr_stats[3], (unsigned long long)__popcll(b3));
                    atomicAdd(&g_scr_stats[4], 1ull);
                    atomicAdd(&g_scr_stats[5], b1 ? 1ull : 0ull);
                    atomicAdd(&g_scr_stats[6], b2 ? 1ull : 0ull);
                    atomicAdd(&g_scr_stats[7], b3 ? 1ull : 0ull);
                    atomicAdd(&g_scr_stats[8], (unsigned long long)__popcll(v1));
                    atomicAdd(&g_scr_stats[9], (unsigned long long)__popcll(v2));
                }
            }
#endif
        }
        const bool act = a_ok && (A.E.lower_only ? a_loc > b_loc : a_loc != b_loc);
        const bool is_sr = test_sr && col_is_sr(M.ci, a_loc);
        if (A.pl_pairs) {
            // a unit with a short-range pair is evaluated whole (its band is dense); otherwise only the candidates themselves
            const bool need_lr = act && !is_sr && do_lr && ms >= lo;
            if (test_sr && __ballot(act && is_sr && keep_sr) != 0ull) bits |= 1u << u;
            else mark_pair(pp, NB - 1, need_lr, q0 + u);
        } else {   // (verify mode: whole units)
            const bool need = act && (is_sr ? keep_sr : (do_lr && ms >= lo));
            if (__ballot(need) != 0ull) bits |= 1u << u;
        }
    }
    return bits;
}

// ------------------------------------------------------------------------------------------------
// Threshold table of the biallelic x biallelic pairs (both SNPs: one indicator row, r = 2).  With the marginals fixed the
// joint table has ONE free number, x = pxy of (minor, minor), and MI is convex in it with its minimum at independence: MI
// reaches a level lo only for x <= L or x >= H.  L and H depend on the two minor marginals alone (RXY >= 1 with equality in the
// intended mode, and MI falls as RXY grows: the table is built for RXY = 1), so they are tabulated once per weighting over
// bins of the two marginals — conservatively: the largest L and the smallest H over the bin (sampled on a 3 x 3 grid, L and H
// ascend with both marginals) — and shifted by everything the approximate sum n' may be off: H (1 - delta) - eta, L (1 + delta)
// + eta, in units of the int32 block.  The screen then dismisses a pair with Lq < n' < Hq on two integer compares and runs the
// 25-cell log evaluation only for the columns in which some lane fails that test (one pair in a few thousand does).
// Every dismissal is still checked in verify mode (ldw_set_screen 2).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double mi11_exact(double x, double pa, double pb, double W, double den) {
    const double A0 = pa + 1.0, A1 = W - pa + 1.0, B0 = pb + 1.0, B1 = W - pb + 1.0;
    const double x01 = A0 - x, x10 = B0 - x, x11 = den - A0 - B0 + x;
    if (!(x > 0.0 && x01 > 0.0 && x10 > 0.0 && x11 > 0.0)) return 1e30;
    return (x * log(x * den / (A0 * B0)) + x01 * log(x01 * den / (A0 * B1)) + x10 * log(x10 * den / (A1 * B0)) + x11 * log(x11 * den / (A1 * B1))) / den;
}

// 32 lanes per bin pair: lanes 0..8 bisect H for one point of the 3 x 3 sample grid each, lanes 16..24 bisect L; lanes 9 and 25 test
// whether the bin can reach the level AT ALL on their side, at the point of the bin where the extreme association carries the most
// information (r05, below); xor-shuffles combine them.  A bisection is a chain of dependent fp64 logarithms — latency, not throughput —
// so the table is built wide: 512 workgroups, 20 steps per lane (always ending on the safe side: fewer steps only loosen a threshold by
// interval / 2^20), cheap enough to rebuild whenever a block's level has drifted (launch_block_apx).
//
// Why the corners suffice for L and H but not for "can the bin reach the level" (r05; tools/fuzz_paths.py --seed 203 --only 96 found two
// perfectly ANTI-associated pairs dismissed at a total weight of 6.6).  d(MI den)/d(pa) at fixed x and pb is log[P(b1|a0) / P(b1|a1)]:
// positive below independence, negative above.  So at fixed x the L side's MI grows with either marginal and the H side's falls: L and H
// both ascend with both marginals, sup L sits at the bin's top corner and inf H at its bottom corner, and where a corner itself cannot reach
// the level its extreme feasible x (xlo of the top corner, xhi of the bottom corner) bounds the others' crossing.  Reachability is a different
// function: MI at the feasibility edge.  On the L side that edge is x = 0 (joint cell empty) while pa + pb <= W and the OPPOSITE cell empty
// beyond; the edge MI ascends with the marginals up to the line pa + pb = W and descends after it, and on the line it is largest where the
// marginals are balanced.  A bin that straddles the line has its best point on the line, strictly inside the bin — r03/r04 judged the L side
// by the nine sample points alone and called such a bin unreachable when the level lay between the samples' edge MI and the line's.  The H
// side mirrors it (swap the labels of b): edge x = min(pa, pb), best point on the diagonal pa = pb nearest to W / 2, which only the diagonal
// bin holding W / 2 can miss between its samples.  Bins are widened by 1e-3 of a bin against the fp32 rounding of tab_bin.
__global__ __launch_bounds__(256) void k_build_tab11(double W, double lo, double delta, double eta, double sprime, int NB, float cbin, int2 *__restrict__ tab) {
    const int gid = blockIdx.x * 256 + threadIdx.x;
    const int id = gid >> 5, role = gid & 31;
    const int smp = role & 15;
    const bool wantL = role >= 16;
    const bool live = id < NB * NB && smp < 10;
    const int idc = id < NB * NB ? id : NB * NB - 1;
    const int jb = idc / NB, ia = idc % NB;   // [bin of the to side][bin of the from side]
    const double den = W + 2.0;
    constexpr double WIDEN = 1e-3;
    double Lmax = -1e30, Hmin = 1e30, XloMax = -1e30;
    bool reach = false;   // this lane's point can reach the level at all on its side
    if (live) {
        // bin k covers sqrt(p) * cbin in [k, k + 1); the last bin is open-ended: it ends at the total weight
        const double ua0 = (ia > 0 ? ia - WIDEN : 0.0) / cbin, ua1 = (ia + 1 + WIDEN) / cbin, ub0 = (jb > 0 ? jb - WIDEN : 0.0) / cbin, ub1 = (jb + 1 + WIDEN) / cbin;
        const double a0 = ua0 * ua0 < W ? ua0 * ua0 : W, b0 = ub0 * ub0 < W ? ub0 * ub0 : W;
        const double a1 = (ia == NB - 1 || ua1 * ua1 > W) ? W : ua1 * ua1, b1 = (jb == NB - 1 || ub1 * ub1 > W) ? W : ub1 * ub1;
        double pa, pb;
        bool have = true;
        if (smp < 9) {
            const int sa = smp / 3, sb = smp % 3;
            pa = sa == 0 ? a0 : (sa == 2 ? a1 : 0.5 * (a0 + a1));
            pb = sb == 0 ? b0 : (sb == 2 ? b1 : 0.5 * (b0 + b1));
        } else if (wantL) {   // the bin's best point for the empty-cell association: on the line pa + pb = W if the bin straddles it
            if (a1 + b1 <= W) { pa = a1; pb = b1; }
            else if (a0 + b0 >= W) { pa = a0; pb = b0; }
            else {
                const double s0 = a0 > W - b1 ? a0 : W - b1, s1 = a1 < W - b0 ? a1 : W - b0;
                pa = 0.5 * W < s0 ? s0 : (0.5 * W > s1 ? s1 : 0.5 * W);
                pb = W - pa;
            }
        } else {              // ... and for the perfect association: on the diagonal if the bin straddles it
            const double s0 = a0 > b0 ? a0 : b0, s1 = a1 < b1 ? a1 : b1;
            have = s0 <= s1;  // (off the diagonal the best point is a corner: sampled)
            pa = pb = 0.5 * W < s0 ? s0 : (0.5 * W > s1 ? s1 : 0.5 * W);
        }
        const double E = (pa + 1.0) * (pb + 1.0) / den;
        double xlo = 0.5, xhi = (pa < pb ? pa : pb) + 0.5;
        const double xmin_feas = (pa + 1.0) + (pb + 1.0) - den + 0.5;
        if (xmin_feas > xlo) xlo = xmin_feas;
        if (smp == 9) {
            reach = have && (wantL ? (E > xlo && mi11_exact(xlo, pa, pb, W, den) >= lo) : (E < xhi && mi11_exact(xhi, pa, pb, W, den) >= lo));
        } else if (!wantL) {
            if (E < xhi && mi11_exact(xhi, pa, pb, W, den) >= lo) {
                double a = E > xlo ? E : xlo, b = xhi;
                for (int it = 0; it < 20; ++it) {
                    const double m = 0.5 * (a + b);
                    if (mi11_exact(m, pa, pb, W, den) < lo) a = m; else b = m;
                }
                Hmin = a;   // MI(a) < lo: everything below a (and above E) is safe
                reach = true;
            } else {
                // r04 (found by the adversarial alignment: a rare state that co-occurs PERFECTLY with a common one — x = xhi, the largest
                // feasible value — was dismissed).  This sample point cannot reach the level even at its largest feasible x = xhi, but a
                // point with larger marginals in the same bin may: an unreachable sample bounds H from below by ITS xhi.
                Hmin = xhi;
            }
        } else {
            XloMax = xlo;   // (the mirror image of the r04 rule: an unreachable sample bounds L from above by ITS xlo)
            if (E > xlo && mi11_exact(xlo, pa, pb, W, den) >= lo) {
                double a = xlo, b = E < xhi ? E : xhi;
                for (int it = 0; it < 20; ++it) {
                    const double m = 0.5 * (a + b);
                    if (mi11_exact(m, pa, pb, W, den) < lo) b = m; else a = m;
                }
                Lmax = b;
                reach = true;
            }
        }
    }
    // lanes 0..15 hold the H side, 16..31 the L side: combine within each half, then across
    int any_reach = reach ? 1 : 0;
#pragma unroll
    for (int off = 1; off <= 8; off <<= 1) {
        const double l2 = __shfl_xor(Lmax, off), h2 = __shfl_xor(Hmin, off), x2 = __shfl_xor(XloMax, off);
        Lmax = l2 > Lmax ? l2 : Lmax;
        Hmin = h2 < Hmin ? h2 : Hmin;
        XloMax = x2 > XloMax ? x2 : XloMax;
        any_reach |= __shfl_xor(any_reach, off);
    }
    if (wantL) Lmax = any_reach ? (XloMax > Lmax ? XloMax : Lmax) : -1e30;
    else Hmin = any_reach ? Hmin : 1e30;
    {
        const double l2 = __shfl_xor(Lmax, 16), h2 = __shfl_xor(Hmin, 16);
        Lmax = l2 > Lmax ? l2 : Lmax;
        Hmin = h2 < Hmin ? h2 : Hmin;
    }
    if (role != 0 || id >= NB * NB) return;
    // n' is at most eta / sprime units below the sum of the approximate weights, which is within delta of the exact sum
    int2 e;
    const double hq = (Hmin * (1.0 - delta) - eta - 0.5) / sprime, lq = (Lmax * (1.0 + delta) + eta - 0.5) / sprime;
    e.y = Hmin > 1e29 ? 2147483647 : (hq < 0.0 ? 0 : (hq > 2147483000.0 ? 2147483647 : (int)floor(hq) - 1));
    e.x = Lmax < -1e29 ? -1 : (lq < -1.0 ? -1 : (lq > 2147483000.0 ? 2147483646 : (int)ceil(lq) + 1));
    tab[id] = e;
}

// biallelic x biallelic columns of the approximate screen through the threshold table
template <int U, int RM>
__device__ __forceinline__ unsigned int screen_cols_tab(const EpiArgs &A, const RowSide &R, int binA, const ColMeta *cmu, int a_loc, bool a_ok, float lo,
                                                        int q0, int tile, PendPairs &pp) {
    const bool test_sr = A.E.any_sr != 0 || A.sr_excl != 0, keep_sr = A.E.keep_sr != 0 && !A.sr_excl;
    int n[U];
    int2 th[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        n[u] = (int)g_entry(A, R, cmu[u]).at(0, 0);
        th[u] = A.tab11[cmu[u].pad2 * A.tab_nb + binA];
    }
    unsigned int bits = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const ColMeta &M = cmu[u];
        const int b_loc = M.bl;
        const bool act = a_ok && (A.E.lower_only ? a_loc > b_loc : a_loc != b_loc);
        const bool is_sr = test_sr && col_is_sr(M.ci, a_loc);
        if (test_sr && __ballot(act && is_sr && keep_sr) != 0ull) {   // a unit with a short-range pair is evaluated whole
            bits |= 1u << u;
            continue;
        }
        const bool maybe = act && !is_sr && !(n[u] > th[u].x && n[u] < th[u].y);
        if (__ballot(maybe) == 0ull) continue;
        // some lane is beyond its thresholds: the full bound for this column
        FullCells<1, 1> C;
        const int64_t v = n[u];
        C.n[0][0] = v;
        C.n[1][0] = M.pb[0] - v;
        C.n[0][1] = R.pa[0] - v;
        C.n[1][1] = R.pa[1] - C.n[1][0];
        const float ms = full_cells_screen<1, 1, true>(A, R, M, screen_rxy(A, R, M, a_loc, b_loc, RM), C);
        const bool need_lr = maybe && ms >= lo;
        const unsigned long long m = __ballot(need_lr);
        if (m == 0ull) continue;
        if (A.pl_pairs) mark_pair(pp, 0, need_lr, q0 + u);   // (both SNPs one indicator row: list 0)
        else bits |= 1u << u;   // verify mode: whole units (the dismissed ones are evaluated too and must not produce anything)
    }
    return bits;
}

// U columns at once for biallelic x biallelic units (4 cells each, the bulk of the work); wider tables go two (or one)
// at a time, which keeps the kernel near 64 VGPRs
template <int NA, int U, int RM, bool APX>
__device__ __forceinline__ unsigned int screen_cols_nb(int nb, const EpiArgs &A, const RowSide &R, const ColMeta *cmu, int a_loc,
                                                       bool a_ok, float lo, int q0, int tile, PendPairs &pp) {
    static_assert(U <= 4, "screen_cols_apx keeps U columns' entries in registers");
    if (APX) return nb == 1 ? screen_cols_apx<NA, 1, U, RM>(A, R, cmu, a_loc, a_ok, lo, q0, tile, pp) : screen_cols_apx<NA, 2, U, RM>(A, R, cmu, a_loc, a_ok, lo, q0, tile, pp);
    if (NA == 1 && nb == 1) return screen_cols<NA, 1, U, RM, APX>(A, R, cmu, a_loc, a_ok, lo, q0, tile, pp);   // (the table path is taken by the caller)
    constexpr int V = LDW_SCREEN_V < U ? LDW_SCREEN_V : U;   // columns in flight for the multi-cell tables (2: 387 -> 372 us per C4 block in r02)
    unsigned int bits = 0;
    for (int u = 0; u < U; u += V) {
        const unsigned int b = nb == 1 ? screen_cols<NA, 1, V, RM, APX>(A, R, cmu + u, a_loc, a_ok, lo, q0 + u, tile, pp)
                                       : screen_cols<NA, 2, V, RM, APX>(A, R, cmu + u, a_loc, a_ok, lo, q0 + u, tile, pp);
        bits |= b << u;
    }
    return bits;
}

// Append the wanted units of a wave (bit k = column slot q_base + k of from-tile `tile`) to the flat list and, in the
// mixed-precision path, to the list of their (tile, row-slot class), which is what the gathered low-limb GEMM walks; the
// index k there tells k_mi_units where the low limbs of the unit's joint sums are.  In verify mode every unit of `all` is
// listed, the unwanted ones marked.
// There are two flat lists: units whose SNPs have 1 or 2 fully flagged slots on both sides (bit set in `fastmask`) go to
// list 0, which the straight-line kernel k_mi_units<true> walks; the others to list 1 (k_mi_units<false>, predicated code).
// units / n_units point at list 0 / its counter; list 1 follows at units + list_stride / n_units + 1.
__device__ __forceinline__ void list_wave_units(const EpiArgs &A, const ColMeta *cm, int c_first, int q_base, int n_it, unsigned int all,
                                                unsigned int wanted, unsigned int fastmask, uint64_t *__restrict__ units,
                                                unsigned int *__restrict__ n_units, int64_t list_stride, int tile = -1) {
    if (tile < 0) tile = (int)blockIdx.x;
    const int lane = threadIdx.x & 63;
    const unsigned int listed = A.E.scr_mode == 2 ? all : wanted;
    if (listed == 0) return;
    const bool mine = lane < 32 && ((listed >> lane) & 1u);
    uint64_t kfield = 0;
    if (A.lo.on) {
        const int my_lc = lane < n_it ? lo_class((int)(cm[c_first + (lane < 32 ? lane : 0)].mb & 7)) : 0;
#pragma unroll
        for (int lc = 0; lc < 3; ++lc) {
            const unsigned int m = (unsigned int)__ballot(mine && my_lc == lc);
            if (m == 0) continue;
            unsigned int base = 0;
            if (lane == 0) base = atomicAdd(&A.lo.cnt[tile * 3 + lc], (unsigned int)__popc(m));
            base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
            if (mine && my_lc == lc) {
                const unsigned int k = base + __popc(m & ((1u << lane) - 1u));
                // bit 31 (verify mode only): a unit the screen dismissed
                A.lo.tl[(int64_t)tile * A.nt + A.lo.uoff[lc] + k] = (uint32_t)(q_base + lane) | (((wanted >> lane) & 1u) ? 0u : 0x80000000u);
                kfield = ((uint64_t)k << 31) | ((uint64_t)lc << 51);
            }
        }
    }
    if (!units) return;   // approximate path: only the per-(tile, class) lists are read (k_units_pop builds the final flat lists)
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        const unsigned int m = listed & (which == 0 ? fastmask : ~fastmask);
        if (m == 0) continue;
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(n_units + which, (unsigned int)__popc(m));
        base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
        if (lane < 32 && ((m >> lane) & 1u)) {
            const uint64_t u = (uint64_t)((uint32_t)tile * (uint32_t)A.nt + (uint32_t)(q_base + lane)) | kfield;
            units[which * list_stride + base + __popc(m & ((1u << lane) - 1u))] = ((wanted >> lane) & 1u) ? u : (u | UNIT_DISMISSED);
        }
    }
}

// RM: how RXY is read (screen_rxy) — a template parameter so that the common square-block code carries neither the
// division nor the table look-ups of the ragged case
// One workgroup's share of the screen: from-tile `tile` (64 SNPs, perm_f order) x column group `cgy` (EPI_COLS column slots, perm_t order).
template <int RM, bool APX>
__device__ __forceinline__ void screen_wg(const EpiArgs &A, const int32_t *__restrict__ perm_f, const int32_t *__restrict__ perm_t,
                                          uint64_t *__restrict__ units, unsigned int *__restrict__ n_units, int64_t list_stride, ColMeta *cm, int tile,
                                          int cgy) {
    const bool square = A.nf == A.nt;
    const bool mixed = A.lo.on != 0 || APX;   // cells derived from the marginals of the weights the block-wide sums were taken with
    if (APX && A.clean && A.E.scr_mode != 2 && tile < A.clean_stride && tile < A.gen_t0) {
        // all four 32-column regions of this workgroup found clean by the GEMM's epilogue: nothing to stage, nothing to list
        bool all_clean = true;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int qb = cgy * EPI_COLS + w * (EPI_COLS / 4);
            const bool whole = qb + EPI_COLS / 4 <= A.nt && qb + EPI_COLS / 4 <= A.gen_q0;
            all_clean = all_clean && whole && A.clean[(int64_t)(qb / 32) * A.clean_stride + tile] != 0;
        }
        if (all_clean) return;
    }
    const int wave = threadIdx.x >> 6;
    const int c_first = wave * (EPI_COLS / 4);
    const int q_base = cgy * EPI_COLS + c_first;
    int n_it = A.nt - q_base;
    n_it = n_it > EPI_COLS / 4 ? EPI_COLS / 4 : n_it;
    // pruning by kind (k_snp_sup): columns whose pairs with EVERY SNP of the tile are dead — the tile's SNPs all dead versus the
    // column's kind, or all of one kind the column's SNP is dead against — are dismissed unread (the approximate GEMM has not
    // even computed most of their sums: apx_tile_prunable).  Not in verify mode, which has to see what is dismissed.  From the
    // flags alone, so that a workgroup with nothing else to do leaves before it stages anything.
    unsigned int dead_cols = 0, tri_cols = 0;
    // Diagonal blocks (lower_only: a pair exists once, with a_loc > b_loc): both epilogue orders keep the list order within a class,
    // so about half of the (tile, column) combinations hold no pair at all — columns whose SNP comes after every SNP of the tile.
    // They used to run the whole bound and mask the result.
    if (A.E.lower_only) {
        int amax = perm_f[tile * 64 + (threadIdx.x & 63)];   // (-1: padding slot)
        const int pb = (int)(threadIdx.x & 63) < n_it ? perm_t[q_base + (threadIdx.x & 63)] : 0x7FFFFFFF;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_xor(amax, off);
            amax = o > amax ? o : amax;
        }
        dead_cols = (unsigned int)__ballot((int)(threadIdx.x & 63) < n_it && pb >= amax);
        tri_cols = dead_cols;
        if (__syncthreads_and((n_it <= 0 || (n_it == EPI_COLS / 4 && dead_cols == 0xFFFFFFFFu)) ? 1 : 0)) return;
    }
    unsigned int prune_cols = 0;   // (in a block with short-range pairs these columns are dropped only where the unit holds none: below)
    if (APX && A.sflag_f && A.E.do_lr) {
        const unsigned fa = A.sflag_f[tile * 64 + (threadIdx.x & 63)];
        const bool real = (fa & PF_PAD) == 0u;   // (a padding slot of the tile: no SNP)
        const unsigned ka = fa & PF_KIND;
        const bool all_k2 = __ballot(real && ka != 2u) == 0ull, all_k3 = __ballot(real && ka != 3u) == 0ull;
        if ((all_k2 || all_k3) && __ballot(real) != 0ull) {
            const bool all_dead2 = __ballot(real && !(fa & PF_DEAD2)) == 0ull, all_dead3 = __ballot(real && !(fa & PF_DEAD3)) == 0ull;
            const unsigned fb = (int)(threadIdx.x & 63) < n_it ? (unsigned)A.sflag_t[q_base + (threadIdx.x & 63)] : 0u;
            const unsigned kb = fb & PF_KIND;
            const bool dead = kb >= 2u && ((kb == 2u ? all_dead2 : all_dead3) || (fb & (all_k2 ? PF_DEAD2 : PF_DEAD3)) != 0u);
            prune_cols = (unsigned int)__ballot(dead);
        }
        if (!A.E.any_sr && A.E.scr_mode != 2) {   // (verify mode lists the pruned units as dismissed: their pairs are checked in fp64 like any other)
            dead_cols |= prune_cols;
            prune_cols = 0;
            const bool wave_done = n_it <= 0 || (n_it == EPI_COLS / 4 && dead_cols == 0xFFFFFFFFu);
            if (__syncthreads_and(wave_done ? 1 : 0)) return;
        }
    }
    stage_cols(A, perm_t, square, cm, mixed, cgy);
    __syncthreads();
    RowSide R;
    int a_loc, na0;
    const bool a_ok = load_row_side(A, perm_f, square, tile, R, a_loc, mixed);
    const bool wave_full = wave_is_full(R, a_ok, na0);
    if (n_it <= 0) return;
    const float lo = (float)A.E.spec_lo - A.E.scr_eps;
    // threshold-table path: every SNP of the tile biallelic with r = 2, long-range pass
    int binA = 0;
    bool use_tab = false;
    if (APX && A.tab11 && A.rowpack && A.E.do_lr && wave_full && na0 == 1) {
        binA = A.rowpack[tile * 64 + (threadIdx.x & 63)].pad;
        use_tab = __ballot(a_ok && R.ra != 2.0) == 0ull;
    }
    // wanted: units that need the fp64 kernel; handled: units this kernel could judge (the others are wanted by default)
    unsigned int wanted = 0, handled = 0;
    PendPairs pp{{0u, 0u}, q_base};
    constexpr int U = 4;
    // from-tiles >= gen_t0 and column slots >= gen_q0 (SNPs with >= 3 minor states, or none) belong to k_mi_screen_generic
    if (tile >= A.gen_t0 || q_base >= A.gen_q0) return;
    if (q_base + n_it > A.gen_q0) n_it = A.gen_q0 - q_base;
    // a region the GEMM's epilogue found clean (every one of its 64 x 32 pairs inside the table thresholds — the very test the
    // table path below would make) is dismissed without a single load
    const bool region_clean = APX && A.clean && n_it == EPI_COLS / 4 && tile < A.clean_stride &&
                              A.clean[(int64_t)(q_base / 32) * A.clean_stride + tile] != 0;
    if (region_clean) {
        handled = 0xFFFFFFFFu;
    } else if (wave_full) {
        for (int it = 0; it < n_it; it += U) {
            if (((dead_cols >> it) & ((1u << U) - 1u)) == ((1u << U) - 1u) && it + U <= n_it && A.E.scr_mode != 2) {
                handled |= ((1u << U) - 1u) << it;
                continue;
            }
            const ColMeta *cmu = &cm[c_first + it];
            if (((((A.E.scr_mode != 2 ? dead_cols : 0u) | prune_cols) >> it) & ((1u << U) - 1u)) == ((1u << U) - 1u) && it + U <= n_it) {
                // prunable columns of a block with short-range pairs: dropped unless the unit holds one (its tile is in the band then)
                bool has_sr = false;
#pragma unroll
                for (int u = 0; u < U; ++u) has_sr = has_sr || col_is_sr(cmu[u].ci, a_loc);
                if (__ballot(a_ok && has_sr) == 0ull) {
                    handled |= ((1u << U) - 1u) << it;
                    continue;
                }
            }
            // the U columns of a group share one code path if they have the same slot count (the rule away from class borders)
            bool same = it + U <= n_it;
            const uint32_t mb0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)cmu[0].mb);
            if (same) {
#pragma unroll
                for (int u = 1; u < U; ++u) {
                    const uint32_t mbu = (uint32_t)__builtin_amdgcn_readfirstlane((int)cmu[u].mb);
                    same = same && (mbu & 7) == (mb0 & 7) && col_is_fast(mbu);
                }
                same = same && col_is_fast(mb0);
            }
            if (same) {
                unsigned int b;
                bool tab_ok = false;
                if (APX && use_tab && (mb0 & 7) == 1) {   // biallelic x biallelic with r = 2 on both sides: the threshold table
                    tab_ok = true;
#pragma unroll
                    for (int u = 0; u < U; ++u) tab_ok = tab_ok && cmu[u].rb == 2.0;
                }
#ifdef LDW_SCREEN_EXP   // timing ablation only (wrong results; profiles/r04_screen_breakdown.txt): bit 0 skips the table path, bit 1 the multi-cell path
                if ((tab_ok && ((LDW_SCREEN_EXP) & 1)) || (!tab_ok && ((LDW_SCREEN_EXP) & 2))) b = 0;
                else
#endif
                if (tab_ok) b = screen_cols_tab<U, RM>(A, R, binA, cmu, a_loc, a_ok, lo, q_base + it, tile, pp);
                else
                    b = na0 == 1 ? screen_cols_nb<1, U, RM, APX>((int)(mb0 & 7), A, R, cmu, a_loc, a_ok, lo, q_base + it, tile, pp)
                                 : screen_cols_nb<2, U, RM, APX>((int)(mb0 & 7), A, R, cmu, a_loc, a_ok, lo, q_base + it, tile, pp);
                wanted |= b << it;
                handled |= ((1u << U) - 1u) << it;
            } else {
                for (int u = 0; u < U && it + u < n_it; ++u) {
                    const uint32_t mbu = (uint32_t)__builtin_amdgcn_readfirstlane((int)cmu[u].mb);
                    if (!col_is_fast(mbu)) continue;
                    const unsigned int b = na0 == 1 ? screen_cols_nb<1, 1, RM, APX>((int)(mbu & 7), A, R, cmu + u, a_loc, a_ok, lo, q_base + it + u, tile, pp)
                                                    : screen_cols_nb<2, 1, RM, APX>((int)(mbu & 7), A, R, cmu + u, a_loc, a_ok, lo, q_base + it + u, tile, pp);
                    wanted |= b << (it + u);
                    handled |= 1u << (it + u);
                }
            }
        }
    }
    if (APX && A.pl_pairs) {   // the pairs this wave marked: lists (na0 - 1) + 2 (nb - 1)
        flush_pairs(A, na0 - 1, pp.m[0], q_base, tile, R.sa, &cm[c_first]);
        flush_pairs(A, na0 + 1, pp.m[1], q_base, tile, R.sa, &cm[c_first]);
    }
    const unsigned int all = n_it >= 32 ? 0xFFFFFFFFu : ((1u << n_it) - 1u);
    if (A.E.scr_mode != 2) handled |= tri_cols;   // (columns without a pair need nobody's attention, whatever the tile looks like; verify mode lists
                                                  // every unit and reads `handled` as "straight-line code applies": left alone there)
    wanted = (wanted | ~handled) & all;
    list_wave_units(A, cm, c_first, q_base, n_it, all, wanted, handled, units, n_units, list_stride, tile);
}


// r04: the entries the GEMM's epilogue found outside their table thresholds (ApxGemmArgs::maybe): one lane per entry evaluates the full
// bound of that ONE pair — what screen_cols_tab does for the columns of a region in which some lane fails the table test — and lists the
// pair if it may reach the block's level.  Both SNPs are biallelic with r = 2 and fully flagged (their rows carry table bins), so a row-list
// position is the epilogue slot: trow = column slot, fcol = 64 * from-tile + lane.  Not used for diagonal blocks or in verify mode.
template <int RM>
__global__ __launch_bounds__(256) void k_screen_maybe(EpiArgs A, const ApxMaybe *__restrict__ maybe, const unsigned int *__restrict__ maybe_n,
                                                      unsigned int maybe_cap) {
    const unsigned int n_all = *maybe_n;
    if (n_all > maybe_cap) {   // the list overflowed: the block takes the pair lists' overflow path — through a word of its own behind the list
        // counters, which k_pick_bucket reads with them (bumping a real counter would make its consumers read entries that were never written)
        if (blockIdx.x == 0 && threadIdx.x == 0) A.pl_n[PH_MAYBE_OVER] = 0xFFFFFFFFu;
        return;
    }
    const float lo = (float)A.E.spec_lo - A.E.scr_eps;
    const bool test_sr = A.E.any_sr != 0 || A.sr_excl != 0;
    // r05: the loop runs wave-uniformly (every lane of a wave makes the same number of trips) and the list append is aggregated per wave and
    // shard.  One atomic per passing LANE on the 8 counters of path 0 was what bound this kernel on data without rare states: 23 M entries and
    // 1.8 M appends per C4 pass took 12 ms (1.3 ms per span); neither the grid size nor 32-byte per-SNP records instead of the full packs moved it.
    const int lane = threadIdx.x & 63;
    const unsigned int stride = gridDim.x * 256u;
    for (unsigned int k0 = blockIdx.x * 256u + (threadIdx.x & ~63u); k0 < n_all; k0 += stride) {
        const unsigned int k = k0 + (unsigned int)lane;
        bool pass = k < n_all;
        ApxMaybe e{0u, 0u, 0};
        int sa = 0, sb = 0;
        if (pass) {
            e = maybe[k];
            // (the _hi packs: integer marginals of the APPROXIMATE weights, the ones n' was summed with — what the screen's cells are derived from;
            // r05: through their 32-byte extracts, the same values — r is a small integer, exact in fp32)
            const MiniCol mc = A.mini_c[e.trow];
            const MiniRow mr = A.mini_r[e.fcol];
            const int a_loc = mr.a_loc, b_loc = mc.bl;
            pass = !(a_loc < 0 || a_loc == b_loc);                            // (padding slot; quirk Q3: an off-diagonal block drops its own diagonal)
            if (pass && test_sr && col_is_sr(A.colpack_hi[e.trow].ci, a_loc)) pass = false;   // (cannot happen: tiles with a short-range pair are never table-tested)
            if (pass) {
                RowSide R;
                ColMeta M;
                R.ra = (double)mr.ra;
                R.rta = (double)mr.rta;
                R.pXf[0] = mr.pX0;
                R.pXf[1] = mr.pX1;
                R.pa[0] = mr.pa0;
                R.pa[1] = mr.pa1;
                M.rb = (double)mc.rb;
                M.rq = (double)mc.rq;
                M.pYf[0] = mc.pY0;
                M.pYf[1] = mc.pY1;
                M.pb[0] = mc.pb0;
                M.ci.pad[1] = mc.seg0;
                sa = mr.sa;
                sb = mc.sb;
                FullCells32<1, 1> C;
                const int v = e.n;
                C.n[0][0] = v;
                C.n[1][0] = (int)M.pb[0] - v;
                C.n[0][1] = (int)R.pa[0] - v;
                C.n[1][1] = (int)R.pa[1] - C.n[1][0];
                const float ms = full_cells_screen<1, 1, true>(A, R, M, screen_rxy(A, R, M, a_loc, b_loc, RM), C);
                pass = ms >= lo;
            }
        }
        if (__ballot(pass) == 0ull) continue;
        const int sub = (int)((e.fcol >> 6) & (PAIR_SHARDS - 1));        // path 0 (1 x 1 indicator rows), sharded by from-tile like append_pairs
        unsigned int pos = 0;
#pragma unroll
        for (int s = 0; s < PAIR_SHARDS; ++s) {
            const unsigned long long m = __ballot(pass && sub == s);
            if (m == 0ull) continue;
            const int leader = __ffsll((long long)m) - 1;
            unsigned int base = 0;
            if (lane == leader) base = atomicAdd(A.pl_n + s, (unsigned int)__popcll(m));
            base = (unsigned int)__shfl((int)base, leader);
            if (pass && sub == s) pos = base + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
        }
        if (pass && pos < A.pl_cap) {
            const int32_t r0a = A.row0[sa], r0b = A.row0[sb];
            PairEnt pe;
            pe.t = e.fcol;
            pe.q = e.trow;
            pe.ra = (uint32_t)r0a | ((uint32_t)(A.row0[sa + 1] - r0a) << 29);
            pe.rb = (uint32_t)r0b | ((uint32_t)(A.row0[sb + 1] - r0b) << 29);
            A.pl_pairs[(int64_t)sub * A.pl_cap + pos] = pe;
        }
    }
}

// the whole grid: one workgroup per (from-tile, column group)
template <int RM, bool APX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LDW_SCREEN_WAVES, 8))) void k_mi_screen(EpiArgs A, const int32_t *__restrict__ perm_f,
                                                                                            const int32_t *__restrict__ perm_t,
                                                                                            uint64_t *__restrict__ units,
                                                                                            unsigned int *__restrict__ n_units,
                                                                                            int64_t list_stride) {
    __shared__ ColMeta cm[EPI_COLS];
    screen_wg<RM, APX>(A, perm_f, perm_t, units, n_units, list_stride, cm, (int)blockIdx.x, (int)blockIdx.y);
}

// ------------------------------------------------------------------------------------------------
// k_mi_screen_generic: the fp32 screen for the units k_mi_screen leaves out — a from-tile or a column whose SNPs have >= 3
// minor states (or none).  Those are 1-2 % of the units, but unscreened they were a quarter of the fp64 kernel's list,
// its slowest entries (predicated code), and a third of the gathered low-limb GEMM.  Launched over the generic
// from-tiles x all columns and over the other tiles x the generic columns.
// ------------------------------------------------------------------------------------------------
struct GenRegions {      // k_mi_screen_generic's two rectangles: a = from-tiles [tile0_a, tile0_a + nt_a) x column groups [0, ncg_a);
    int tile0_a, nt_a, ncg_a;   // b = from-tiles [0, nt_b) x ncg_b column groups from column slot q0_b
    int nt_b, q0_b, ncg_b;
};
constexpr int GEN_COLS = 16;   // column slots per workgroup of k_mi_screen_generic: 4 per wave — the kernel is a chain of
                               // dependent loads per column with nothing else to hide them, so the chains are kept short
template <bool APX>
__global__ __launch_bounds__(256) void k_mi_screen_generic(EpiArgs A, const int32_t *__restrict__ perm_f, const int32_t *__restrict__ perm_t,
                                                           uint64_t *__restrict__ units, unsigned int *__restrict__ n_units,
                                                           int64_t list_stride, GenRegions Rg) {
    __shared__ ColMeta cm[GEN_COLS];
    const bool square = A.nf == A.nt;
    const bool mixed = A.lo.on != 0 || APX;
    // both regions in ONE launch (1-D grid): the generic from-tiles x all columns, then the other tiles x the generic columns
    int bid = (int)blockIdx.x, tile, qb;
    if (bid < Rg.nt_a * Rg.ncg_a) {
        tile = Rg.tile0_a + bid % Rg.nt_a;
        qb = (bid / Rg.nt_a) * GEN_COLS;
    } else {
        bid -= Rg.nt_a * Rg.ncg_a;
        tile = bid % Rg.nt_b;
        qb = Rg.q0_b + (bid / Rg.nt_b) * GEN_COLS;
    }
    if (threadIdx.x < GEN_COLS) {
        const int q = qb + (int)threadIdx.x;
        if (q < A.nt) {
            ColMeta m;
            load_col(A, perm_t, square, q, m, mixed);
            cm[threadIdx.x] = m;
        }
    }
    __syncthreads();
    RowSide R;
    int a_loc;
    const bool a_ok = load_row_side(A, perm_f, square, tile, R, a_loc, mixed);
    const int wave = threadIdx.x >> 6;
    const int c_first = wave * (GEN_COLS / 4);
    const int q_base = qb + c_first;
    int n_it = A.nt - q_base;
    n_it = n_it > GEN_COLS / 4 ? GEN_COLS / 4 : n_it;
    if (n_it <= 0) return;
    const int rxy_mode = rxy_read_mode(A.quirk, A.span, square);
    const float lo = (float)A.E.spec_lo - A.E.scr_eps;
    const bool test_sr = A.E.any_sr != 0 || A.sr_excl != 0, keep_sr = A.E.keep_sr != 0 && !A.sr_excl, do_lr = A.E.do_lr != 0;
    unsigned int wanted = 0, mine = 0;   // mine: the units of this wave that belong to this kernel
    PendPairs pp{{0u, 0u}, q_base};
    for (int it = 0; it < n_it; ++it) {
        // the same split as k_mi_screen's: its domain is tile < gen_t0 and q < gen_q0, where it takes the fast units and
        // lists the others unscreened (unflagged slots); everything outside that domain is screened here
        if (tile < A.gen_t0 && q_base + it < A.gen_q0) continue;
        const ColMeta &M = cm[c_first + it];
        mine |= 1u << it;
        const int b_loc = M.bl;
        const bool act = a_ok && (A.E.lower_only ? a_loc > b_loc : a_loc != b_loc);
        const double rxy = screen_rxy(A, R, M, a_loc, b_loc, rxy_mode);
        const float ms = do_lr ? pair_screen_generic<APX>(A, R, M, rxy, g_entry(A, R, M)) : 0.0f;
        const bool is_sr = test_sr && col_is_sr(M.ci, a_loc);
        if (APX && A.pl_pairs) {
            const bool need_lr = act && !is_sr && do_lr && ms >= lo;
            if (__ballot(act && is_sr && keep_sr) != 0ull) {
                wanted |= 1u << it;
            } else {
                mark_pair(pp, 0, need_lr, q_base + it);
            }
        } else {
            const bool need = act && (is_sr ? keep_sr : (do_lr && ms >= lo));
            if (__ballot(need) != 0ull) wanted |= 1u << it;
        }
    }
    if (APX && A.pl_pairs) flush_pairs(A, 4, pp.m[0], q_base, tile, R.sa, &cm[c_first]);   // (the predicated list)
    list_wave_units(A, cm, c_first, q_base, n_it, mine, wanted & mine, 0u, units, n_units, list_stride, tile);
}

// would this pair leave a trace (short-range row or long-range candidate)?  Verify mode of the screen only.
__device__ __forceinline__ bool would_emit(const EmitArgs &E, const ColInfo &c, int a_loc, int b_loc, double mi) {
    if (pair_seg(a_loc, b_loc, E.lower_only) < 0) return false;
    if (E.any_sr && col_is_sr(c, a_loc)) return E.keep_sr != 0;
    return E.do_lr && mi >= E.spec_lo && mi_bucket(mi) >= E.spec_B;
}

// MI of one pair by the variant that fits the slot counts (wave-uniform choice)
__device__ __forceinline__ double unit_pair_mi(const EpiArgs &A, const RowSide &R, const ColMeta &M, int a_loc, int b_loc, bool square,
                                               bool fast, int na0, int na_max, int nb, const GAcc &Ga) {
    if (fast) {
        if (na0 == 1) return nb == 1 ? pair_mi_full<1, 1>(A, R, M, a_loc, b_loc, square, Ga) : pair_mi_full<1, 2>(A, R, M, a_loc, b_loc, square, Ga);
        return nb == 1 ? pair_mi_full<2, 1>(A, R, M, a_loc, b_loc, square, Ga) : pair_mi_full<2, 2>(A, R, M, a_loc, b_loc, square, Ga);
    }
    if (na_max == 1) {
        if (nb <= 1) return pair_mi<1, 1>(A, R, M, a_loc, b_loc, square, Ga);
        if (nb == 2) return pair_mi<1, 2>(A, R, M, a_loc, b_loc, square, Ga);
        return pair_mi<1, 4>(A, R, M, a_loc, b_loc, square, Ga);
    }
    if (na_max == 2) {
        if (nb <= 1) return pair_mi<2, 1>(A, R, M, a_loc, b_loc, square, Ga);
        if (nb == 2) return pair_mi<2, 2>(A, R, M, a_loc, b_loc, square, Ga);
        return pair_mi<2, 4>(A, R, M, a_loc, b_loc, square, Ga);
    }
    if (nb <= 1) return pair_mi<4, 1>(A, R, M, a_loc, b_loc, square, Ga);
    if (nb == 2) return pair_mi<4, 2>(A, R, M, a_loc, b_loc, square, Ga);
    return pair_mi<4, 4>(A, R, M, a_loc, b_loc, square, Ga);
}


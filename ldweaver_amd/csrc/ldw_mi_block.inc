// Part of ldw_mi.hip (inside its anonymous namespace): host side of ONE block — row lists and short-range intervals (build_side, build_cols),
// list capacities, the plain / mixed chain (launch_block_mi), the approximate-GEMM chain in two phases (launch_block_apx), ldw_mi_block's
// driver, the link tables' capacity and the layout of the small device-side records.

int upload_i32(ldw_ctx *c, ldw::DevBuf &buf, const std::vector<int32_t> &v) {
    if (int rc = buf.reserve(v.size() * 4 + 4)) return rc;
    if (!v.empty()) LDW_HIP(hipMemcpyAsync(buf.p, v.data(), v.size() * 4, hipMemcpyHostToDevice, c->stream));
    return LDW_OK;
}

// Row list of one side of a block.  SNPs are grouped by slot-count CLASS — 1, 2 or 4 indicator rows after padding
// (0 -> 1, 3 -> 4 with rows of zeros) — in their list order within a class, and every class starts on a 32-row
// boundary: a 32 x 32 MFMA tile then holds whole SNPs of one class on either side and no SNP straddles the 64 x 32
// sub-tile of a wave.  lrow[k] = row
// position of SNP k's first row; pos[p] = k at that position, -1 elsewhere; cls[g] = class of 32-row group g.
struct SideLists {
    std::vector<int32_t> rowlist, lrow, pos;
    std::vector<uint8_t> cls;
    int Rpad = 0;
};

// order1 (optional): the list positions of the SNPs of class 1 in the order their rows are to take (prep_block: by the weight of
// the minor state); the other classes, and class 1 without it, keep the list order.
int build_side(ldw_ctx *c, const int32_t *idx, int64_t n, SideLists &S, const std::vector<int32_t> *order1 = nullptr) {
    S.lrow.assign((size_t)n, 0);
    S.rowlist.clear();
    S.pos.clear();
    S.cls.clear();
    const int32_t zero_row = (int32_t)c->rows.R;   // rows R .. R+TILE-1 of Mbits are zero
    for (int64_t k = 0; k < n; ++k)
        LDW_REQUIRE(idx[k] >= 0 && idx[k] < c->L, LDW_ERR_ARG, "SNP index %d out of range 0..%lld", idx[k], (long long)c->L - 1);
    for (int cl : {1, 2, 4}) {
        const bool ordered = cl == 1 && order1 != nullptr;
        const int64_t cnt = ordered ? (int64_t)order1->size() : n;
        for (int64_t kk = 0; kk < cnt; ++kk) {
            const int64_t k = ordered ? (int64_t)(*order1)[(size_t)kk] : kk;
            const int32_t a = idx[k];
            const int nr = c->rows.h_row0[a + 1] - c->rows.h_row0[a];
            const int mine = nr <= 1 ? 1 : (nr == 2 ? 2 : 4);
            if (mine != cl) continue;
            S.lrow[k] = (int32_t)S.rowlist.size();
            for (int q = 0; q < cl; ++q) {
                S.rowlist.push_back(q < nr ? c->rows.h_row0[a] + q : zero_row);
                S.pos.push_back(q == 0 ? (int32_t)k : -1);
            }
        }
        while (S.rowlist.size() % 32) {
            S.rowlist.push_back(zero_row);
            S.pos.push_back(-1);
        }
        S.cls.resize(S.rowlist.size() / 32, (uint8_t)cl);
    }
    int64_t rp = ((int64_t)S.rowlist.size() + TILE - 1) / TILE * TILE;
    if (rp == 0) rp = TILE;
    LDW_REQUIRE(rp < 2000000000LL, LDW_ERR_ARG, "block too large");
    S.rowlist.resize((size_t)rp, zero_row);
    S.pos.resize((size_t)rp, -1);
    S.cls.resize((size_t)rp / 32, (uint8_t)1);
    S.Rpad = (int)rp;
    return LDW_OK;
}

// Short-range intervals of every to-side SNP (host, O(nt log nf)); returns the block's short-range row count.
// Requires the from-side list to be ascending in POS (true for contiguous blocks and for the order-preserving
// subsets of SR-only mode).  The intervals come from three position windows, which are exact when the positions
// of both sides lie within one turn of the circle (within_one_turn, ldw_pass_plan.h); the predicate of the
// reference (circ_len <= sr_dist) is then evaluated at the interval boundaries only, as a guard on the window
// arithmetic — it proves nothing about the inside of an interval — and a column that fails it is rebuilt by
// scanning.  A block whose positions do NOT lie within one turn (positions beyond g: a window can then begin
// and end on partners and hold non-partners inside) builds every column by that scan and takes no quick reject.
int build_cols(ldw_ctx *c, const int32_t *from_idx, int64_t nf, const int32_t *to_idx, int64_t nt, bool diag, double sr_dist,
               std::vector<ColInfo> &cols, int64_t &n_sr_blk) {
    const double g = c->meta.g;
    std::vector<double> pf((size_t)nf);
    for (int64_t a = 0; a < nf; ++a) {
        pf[a] = (double)c->meta.h_POS[from_idx[a]];
        LDW_REQUIRE(a == 0 || pf[a] >= pf[a - 1], LDW_ERR_ARG, "from-side SNP list must be ascending in POS (position %lld)", (long long)a);
    }
    cols.resize((size_t)nt);
    bool one_turn = true;
    {   // quick reject: when the two position ranges are farther apart than sr_dist both directly and around the
        // origin, no pair of the block is short-range (true for most off-diagonal blocks)
        double pt_min = (double)c->meta.h_POS[to_idx[0]], pt_max = pt_min;
        for (int64_t b = 1; b < nt; ++b) {
            const double v = (double)c->meta.h_POS[to_idx[b]];
            pt_min = v < pt_min ? v : pt_min;
            pt_max = v > pt_max ? v : pt_max;
        }
        const double pf_min = pf.front(), pf_max = pf.back();
        const bool apart = (pt_min - pf_max > sr_dist && pf_min + g - pt_max > sr_dist) ||
                           (pf_min - pt_max > sr_dist && pt_min + g - pf_max > sr_dist);
        one_turn = within_one_turn(std::min(pf_min, pt_min), std::max(pf_max, pt_max), g);
        if (one_turn && apart && 2 * sr_dist < g) {
            ColInfo z;
            memset(&z, 0, sizeof(z));
            std::fill(cols.begin(), cols.end(), z);
            n_sr_blk = 0;
            return LDW_OK;
        }
    }
    int64_t total_u = 0, total_l = 0;
    std::vector<int32_t> cu((size_t)nt), cl((size_t)nt);
    // The four window bounds of a column are those of std::lower_bound / std::upper_bound over pf.  POS ascends along the to side of every block
    // the item pipeline prepares, so each bound only moves forward from the previous column's: a walk, O(nf + nt) for the block instead of four
    // binary searches per column (0.4 of the 1.2 ms a 10k x 10k diagonal block took to prepare — the first item of a pass, which the GPU waits
    // for).  A column whose position steps back searches afresh; the results are the same either way.
    int64_t hint[4] = {0, 0, 0, 0};
    double p_prev = 0;
    for (int64_t b = 0; b < nt; ++b) {
        const double p1 = (double)c->meta.h_POS[to_idx[b]];
        const bool fwd = b > 0 && p1 >= p_prev;
        p_prev = p1;
        auto lower = [&](int64_t &h, double v) -> int64_t {   // first index with pf >= v
            if (!fwd) h = std::lower_bound(pf.begin(), pf.end(), v) - pf.begin();
            else while (h < nf && pf[(size_t)h] < v) ++h;
            return h;
        };
        auto upper = [&](int64_t &h, double v) -> int64_t {   // first index with pf > v
            if (!fwd) h = std::upper_bound(pf.begin(), pf.end(), v) - pf.begin();
            else while (h < nf && pf[(size_t)h] <= v) ++h;
            return h;
        };
        auto P = [&](int64_t a) { return circ_len(p1, pf[a], g) <= sr_dist; };
        ColInfo ci;
        memset(&ci, 0, sizeof(ci));
        // candidate intervals from the three position windows
        int64_t iv[3][2];
        iv[0][0] = 0;                                                                                // wrap-low: x <= p1 + sr - g
        iv[0][1] = upper(hint[0], p1 + sr_dist - g);
        iv[1][0] = lower(hint[1], p1 - sr_dist);               // centre
        iv[1][1] = upper(hint[2], p1 + sr_dist);
        iv[2][0] = lower(hint[3], p1 - sr_dist + g);           // wrap-high
        iv[2][1] = nf;
        // merge overlapping / touching intervals, keep ascending order
        int n = 0;
        int64_t m[3][2];
        for (int k = 0; k < 3; ++k) {
            if (iv[k][1] <= iv[k][0]) continue;
            if (n > 0 && iv[k][0] <= m[n - 1][1]) m[n - 1][1] = std::max(m[n - 1][1], iv[k][1]);
            else { m[n][0] = iv[k][0]; m[n][1] = iv[k][1]; ++n; }
        }
        bool ok = one_turn;
        for (int k = 0; k < n && ok; ++k) {
            ok = P(m[k][0]) && P(m[k][1] - 1);
            if (ok && m[k][0] > 0) ok = !P(m[k][0] - 1);
            if (ok && m[k][1] < nf) ok = !P(m[k][1]);
        }
        if (ok && n == 0 && nf > 0) ok = !P(0) && !P(nf - 1);
        if (!ok) {  // rebuild from the exact predicate
            n = 0;
            int64_t a = 0;
            while (a < nf) {
                if (!P(a)) { ++a; continue; }
                int64_t e = a;
                while (e < nf && P(e)) ++e;
                LDW_REQUIRE(n < 3, LDW_ERR_ARG, "short-range partners of SNP %d form more than three index runs", to_idx[b]);
                m[n][0] = a; m[n][1] = e; ++n;
                a = e;
            }
        }
        for (int k = 0; k < 3; ++k) {
            ci.s[k] = k < n ? (int32_t)m[k][0] : 0;
            ci.e[k] = k < n ? (int32_t)m[k][1] : 0;
        }
        cu[b] = diag ? 0 : col_count(ci, 0, (int)std::min<int64_t>(b, nf));
        cl[b] = col_count(ci, (int)std::min<int64_t>(b + 1, nf), (int)nf);
        total_u += cu[b];
        total_l += cl[b];
        cols[b] = ci;
    }
    // row order of the block: all upper-segment columns, then all lower-segment columns (R/computePairwiseMI.R:306-310)
    int64_t ru = 0, rl = total_u;
    for (int64_t b = 0; b < nt; ++b) {
        cols[b].off_u = ru;
        cols[b].off_l = rl;
        ru += cu[b];
        rl += cl[b];
    }
    n_sr_blk = total_u + total_l;
    return LDW_OK;
}

bool same_list(const int32_t *a, int64_t na, const int32_t *b, int64_t nb) {
    if (na != nb) return false;
    for (int64_t i = 0; i < na; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

// device pointers of one block's index structures
struct DevPtrs {
    const int32_t *idx_f, *idx_t, *rl_f, *rl_t, *lrow_f, *lrow_t, *perm, *perm_t, *pos_f, *pos_t;
    const ColInfo *cols;        // short-range intervals of every to-side SNP (build_cols)
    const uint8_t *cls_f, *cls_t;
    const int32_t *cmax_f;      // mixed-precision path: per from-tile widest row-slot class, offsets of the low-limb blocks
    const int64_t *tile_base;
    const int32_t *tf_list;     // (tile, fs) pairs of the gathered GEMM's grid
    const uint8_t *band_mask;   // approximate path: [RTpad / 128][RFpad / 64] exact-GEMM tiles that hold a short-range pair
    const uint32_t *band_list;  // r06: the same tiles as a list (by << 16 | bx; a diagonal block's tiles above the diagonal left out), n_band of them; null: none
    int n_band;
    int nf_tiles;               // tiles of 64 in the padded from-side order perm
    int gen_t0, gen_q0;         // first from-tile / column slot of the SNPs with >= 3 minor states or none (k_mi_screen_generic)
};

// host half of LoGeom
struct LoHost {
    int32_t n_lc[3] = {0, 0, 0}, uoff[3] = {0, 0, 0}, rowbase[3] = {0, 0, 0};
    int32_t RTlo = 0, ntiles = 0, n_tf = 0;
    int64_t glo_total = 0;
    int32_t n_tiles_cf[3] = {0, 0, 0};   // from-tiles whose widest row-slot class is 1, 2, 4
    int band_full = 0;                   // the exact GEMM has to cover every tile (a SNP with unflagged slots: its units are not screened)
    int apx = 0, slot = 0, diag = 0;     // approximate-GEMM path (ldw_apx.h) instead of the high-limb GEMM + gathered low limbs
    int ordered = 0;                     // rows of the one-row SNPs in order of the minor state's weight (prep_block: tile pruning)
    int fuse_ok = 0;                     // rows of one-row SNPs sit at their slot index in both row lists (no SNP without a row): the
                                         // GEMM's epilogue may apply the threshold table by row (ApxGemmArgs::fuse)
    int span = 0;                        // reference blocks on the to side (0: an ordinary block); sseg: their candidate lists / histograms
    const SpanSeg *sseg = nullptr;
    // r04: the threshold table this item's FIRST phase chose (null: none applies) — its second phase, queued after the first phases of later
    // items (which may rebuild the table for their level), takes exactly this one
    mutable const int2 *tab_p = nullptr;
    mutable bool tab_set = false;
};

void fill_epi_args(ldw_ctx *c, const DevPtrs &D, int64_t nf, int64_t nt, int RFpad, int quirk, const EmitArgs &E, const int64_t *G,
                   EpiArgs &A) {
    A.G = G;
    A.mini_c = nullptr;
    A.mini_r = nullptr;
    A.RFpad = RFpad;
    A.RTpad = 0;
    A.idx_f = D.idx_f;
    A.lrow_f = D.lrow_f;
    A.idx_t = D.idx_t;
    A.lrow_t = D.lrow_t;
    A.nf = (int)nf;
    A.nt = (int)nt;
    A.slot_meta = c->rows.slot_meta.as<uint32_t>();
    A.slot_pfix = c->rows.slot_pfix.as<int64_t>();
    A.r = c->meta.r.as<double>();
    A.neff = c->wts.neff;
    A.scale = std::ldexp(1.0, -c->wts.frac_bits);
    A.quirk = quirk;
    A.gen_t0 = D.gen_t0;
    A.gen_q0 = D.gen_q0;
    A.colpack = A.colpack_hi = nullptr;
    A.rowpack = A.rowpack_hi = nullptr;
    A.rloc_f = A.rloc_t = nullptr;
    A.pl_pairs = nullptr;
    A.pl_n = nullptr;
    A.pl_cap = 0;
    A.row0 = c->rows.row0.as<int32_t>();
    A.tab11 = nullptr;
    A.clean = nullptr;
    A.clean_stride = 0;
    A.sflag_f = A.sflag_t = nullptr;
    A.snp_sup = nullptr;
    A.tab_nb = 0;
    A.tab_c = 0;
    A.span = 0;
    A.sr_excl = 0;
    memset(A.sseg, 0, sizeof(A.sseg));
    A.E = E;
    memset(&A.lo, 0, sizeof(A.lo));
}

// GEMM + epilogue (or the histogram engine) of one block into ctx->MIblk; with E.cols set, the short-range
// scatter and the long-range histogram ride along.  Everything is asynchronous.
// stage events per block: [0] GEMM start, [1] GEMM end (GEMM stream); [4] epilogue start, [2] epilogue end, [3] selection
// end (main stream).  The GEMM of block b+1 runs beside the epilogue and selection of block b, so the stage times overlap.
constexpr int EVB = 6;
// which: 1 = GEMM only (on gstream, into Gbuf), 2 = epilogue only, 3 = both
constexpr int HI_LIMBS = 3, LO_LIMBS = 2;   // mixed-precision split of the 5 weight limbs
// capacity of the pair lists of one block: pair_cap_of (ldw_slots.h), or g_pair_cap_override (ldw_set_pair_cap, tests only): a fixed small capacity, so
// that the overflow fallback can be exercised.
static std::atomic<uint32_t> g_pair_cap_override{0};
inline uint32_t pair_cap_for(int64_t nf, int64_t nt, int nseg = 0) {
    const uint32_t ovr = g_pair_cap_override.load();
    if (ovr) return ovr;
    return pair_cap_of(nf, nt, nseg);
}
// entries of the maybe list of an item (ApxGemmArgs::maybe): maybe_cap_of (ldw_slots.h), the worst case, so the list cannot overflow whatever the data
// look like.  r04 sized it for "one pair in a few thousand fails its table thresholds" (nf nt / 256 + 65 536), which holds on alignments full
// of rare states; on an alignment without them (MAF 0.2-0.5: the bench's adversarial leg) most regions hand over tens of entries, the list
// overflowed on nearly every block and each of them was redone on the plain path — 216 ms per pass against 155 ms for the plain path itself.
inline uint32_t maybe_cap_for(int64_t RTpad, int64_t RFpad) {
    if (const char *e = getenv("LDW_MAYBE_CAP")) {   // (tests: a list that overflows makes its block take the pair lists' overflow path)
        const long k = atol(e);
        if (k > 0) return (uint32_t)k;
    }
    return maybe_cap_of(RTpad, RFpad);
}
// a block (or a span's segment) redone because a list overflowed (PickOut::over): counted, and a maybe list that overflowed — impossible at its
// worst-case capacity, so only under LDW_MAYBE_CAP — is switched off for the rest of the pass instead of overflowing item after item
inline void note_overflow(ldw_ctx *c, int over) {
    if (over & 1) ++c->cnt.pair_list_overflows;
    if (over & 2) {
        ++c->cnt.maybe_overflows;
        c->spec.maybe_off = true;
    }
}
// The run-time RXY read mode (rxy_read_mode, ldw_epi.h) as a template argument: f(std::integral_constant<int, RM>).  SPAN = false leaves mode 3 out:
// the chain of launch_block_mi runs no span, and its screen is not instantiated for one.
template <bool SPAN = true, class F> void with_rxy_mode(int rm, F &&f) {
    if (rm == 0) f(std::integral_constant<int, 0>{});
    else if (rm == 1) f(std::integral_constant<int, 1>{});
    else if (rm == 2 || !SPAN) f(std::integral_constant<int, 2>{});
    else if constexpr (SPAN) f(std::integral_constant<int, 3>{});
}
// the units outside k_mi_screen's domain, in one launch over both regions: generic from-tiles x all columns, the other tiles x the generic columns
template <bool APX> void launch_screen_generic(const EpiArgs &A, const DevPtrs &D, int n_tiles, const UnitsLayout &U, hipStream_t st) {
    const int gt0 = std::min<int>(A.gen_t0, n_tiles);
    GenRegions Rg;
    Rg.tile0_a = gt0;
    Rg.nt_a = n_tiles - gt0;
    Rg.ncg_a = Rg.nt_a > 0 ? (A.nt + GEN_COLS - 1) / GEN_COLS : 0;
    Rg.nt_b = (gt0 > 0 && A.gen_q0 < A.nt) ? gt0 : 0;
    Rg.q0_b = std::min<int>(A.gen_q0, A.nt) / GEN_COLS * GEN_COLS;
    Rg.ncg_b = Rg.nt_b > 0 ? (A.nt - Rg.q0_b + GEN_COLS - 1) / GEN_COLS : 0;
    const long long nblk = (long long)Rg.nt_a * Rg.ncg_a + (long long)Rg.nt_b * Rg.ncg_b;
    if (nblk > 0)
        hipLaunchKernelGGL(k_mi_screen_generic<APX>, dim3((unsigned)nblk), dim3(256), 0, st, A, D.perm, D.perm_t, U.flat, U.counters, U.list_stride, Rg);
}
// the fp64 MI of the listed units: the straight-line code over the first flat list, the predicated code over the second
void launch_units(const EpiArgs &A, const DevPtrs &D, const UnitsLayout &U, unsigned long long *ghist, hipStream_t st) {
    UnitLists UL;
    memset(&UL, 0, sizeof(UL));
    UL.units[0] = U.flat;
    UL.n[0] = U.counters;
    hipLaunchKernelGGL(k_mi_units<true>, dim3(2048, 1), dim3(256), 0, st, A, D.perm, D.perm_t, UL, ghist);
    UnitLists UG;
    memset(&UG, 0, sizeof(UG));
    UG.units[0] = U.flat + U.list_stride;
    UG.n[0] = U.counters + 1;
    hipLaunchKernelGGL(k_mi_units<false>, dim3(512, 1), dim3(256), 0, st, A, D.perm, D.perm_t, UG, ghist);
}
// the per-block SNP constants k_build_packs wrote (it runs with none set: it derives what the packs then hold); hi: the screen reads the _hi copies
void bind_packs(EpiArgs &A, const PacksLayout &K, bool hi) {
    A.rloc_f = K.rloc_f;
    A.rloc_t = K.rloc_t;
    A.colpack = K.cp;
    A.colpack_hi = hi ? K.cp_hi : K.cp;
    A.rowpack = K.rp;
    A.rowpack_hi = hi ? K.rp_hi : K.rp;
}
int launch_block_mi(ldw_ctx *c, const DevPtrs &D, int64_t nf, int64_t nt, int RFpad, int RTpad, int quirk, EmitArgs E,
                    const hipEvent_t *ev, int which, ldw::DevBuf *Gb, hipStream_t gstream, unsigned long long *ghist,
                    const LoHost *mixed = nullptr) {
    ldw::DevBuf &Gbuf = Gb ? *Gb : c->G;
    if (!gstream) gstream = c->stream;
    if (which == 1) {   // the GEMM of a block, possibly on its own stream so that it overlaps the previous block's tail
        if (int rc = Gbuf.reserve((size_t)RFpad * RTpad * 8)) return rc;
        LDW_HIP(hipEventRecord(ev[0], gstream));
        // mixed-precision path: the block-wide GEMM carries the high limbs only
        if (int rc = launch_gemm_bits(c, c->rows.Mbits.as<uint64_t>(), c->KW, D.rl_t, RTpad, D.rl_f, RFpad, Gbuf.as<int64_t>(),
                                      mixed ? HI_LIMBS : c->wts.nlimbs, c->wts.digits.as<int8_t>() + (mixed ? (int64_t)LO_LIMBS * c->KW * 64 : 0),
                                      E.lower_only, gstream))
            return rc;
        LDW_HIP(hipEventRecord(ev[1], gstream));
        LDW_HIP(hipEventRecord(ev[5], gstream));
        return LDW_OK;
    }
    const bool epilogue_only = which == 2;
    if (int rc = c->MIblk.reserve((size_t)nf * nt * 8)) return rc;
    E.MI = c->MIblk.as<double>();
    E.nf = (int)nf;
    dim3 egrid((unsigned)(D.nf_tiles > 0 ? D.nf_tiles : (nf + 63) / 64), (unsigned)((nt + EPI_COLS - 1) / EPI_COLS));
    LDW_REQUIRE(egrid.y <= 65535u, LDW_ERR_ARG, "nt too large for the epilogue grid");
    if (!epilogue_only) {
        if (int rc = Gbuf.reserve((size_t)RFpad * RTpad * 8)) return rc;
        LDW_HIP(hipEventRecord(ev[0], c->stream));
        if (c->knobs.engine == LDW_ENGINE_HIST) {   // the histogram formulation on bit planes: class-wise popcounts instead of the MFMA GEMM
            if (int rc = launch_cooc_popc(c, D.rl_t, RTpad, D.rl_f, RFpad, Gbuf.as<int64_t>(), E.lower_only, c->stream)) return rc;
        } else if (int rc = launch_gemm_bits(c, c->rows.Mbits.as<uint64_t>(), c->KW, D.rl_t, RTpad, D.rl_f, RFpad, Gbuf.as<int64_t>(), c->wts.nlimbs,
                                             c->wts.digits.as<int8_t>(), E.lower_only, c->stream))
            return rc;
        LDW_HIP(hipEventRecord(ev[1], c->stream));
    }
    EpiArgs A;
    fill_epi_args(c, D, nf, nt, RFpad, quirk, E, Gbuf.as<int64_t>(), A);
    if (which == 2) LDW_HIP(hipEventRecord(ev[4], c->stream));
    if (A.E.scr_mode && A.E.cols && !A.E.write_dense) {
        // speculative mode: the lean fp32 screen lists the units that need the exact value, k_mi_units evaluates those
        const SlotGeom g{nf, nt, RFpad, RTpad, (int64_t)egrid.x, 0, mixed != nullptr};
        UnitsLayout U(g);
        if (int rc = U.reserve(c->scr_units)) return rc;
        LDW_HIP(hipMemsetAsync(U.zeroed().p, 0, U.zeroed().bytes, c->stream));
        if (mixed) {
            LDW_REQUIRE(mixed->ntiles == (int)egrid.x, LDW_ERR_STATE, "mixed-precision geometry does not match the epilogue grid");
            if (int rc = ensure_hi_marginals(c)) return rc;
            if (int rc = c->glo.reserve((size_t)mixed->glo_total * 4 + 64)) return rc;
            LoGeom &lo = A.lo;
            for (int k = 0; k < 3; ++k) {
                lo.n_lc[k] = mixed->n_lc[k];
                lo.uoff[k] = mixed->uoff[k];
                lo.rowbase[k] = mixed->rowbase[k];
            }
            lo.RTlo = mixed->RTlo;
            lo.ntiles = mixed->ntiles;
            lo.on = 1;
            lo.cmax_f = D.cmax_f;
            lo.tile_base = D.tile_base;
            lo.cnt = U.tile_cnt();
            lo.tl = U.tl;
            lo.glo = c->glo.as<int32_t>();
            lo.slot_pfix_hi = c->rows.slot_pfix_hi.as<int64_t>();
            lo.hi_shift = 8 * LO_LIMBS;
        }
        {   // per-block SNP constants in epilogue order (A.lo is final by now: the high-limb marginals are reachable)
            PacksLayout K(g);
            if (int rc = K.reserve(c->packs)) return rc;
            const int nthr = std::max<int>((int)nt, (int)g.nf_slots());
            hipLaunchKernelGGL(k_build_packs, dim3((unsigned)((nthr + 255) / 256), 2), dim3(256), 0, c->stream, A, D.perm, D.perm_t, (int)g.nf_slots(),
                               mixed ? 1 : 0, K.cp, K.cp_hi, K.rp, K.rp_hi, K.rloc_f, K.rloc_t);
            LDW_HIP(hipGetLastError());
            bind_packs(A, K, mixed != nullptr);
        }
        with_rxy_mode<false>(rxy_read_mode(quirk, 0, nf == nt), [&](auto RM) {
            hipLaunchKernelGGL((k_mi_screen<decltype(RM)::value, false>), egrid, dim3(256), 0, c->stream, A, D.perm, D.perm_t, U.flat, U.counters, U.list_stride);
        });
        LDW_HIP(hipGetLastError());
        launch_screen_generic<false>(A, D, (int)egrid.x, U, c->stream);
        LDW_HIP(hipGetLastError());
        if (mixed) {   // low limbs of the listed units
            LoGemmArgs P;
            P.Mbits = c->rows.Mbits.as<uint64_t>();
            P.KW = c->KW;
            P.Kpad = c->KW * 64;
            P.digits_lo = c->wts.digits.as<int8_t>();
            P.perm_f = D.perm;
            P.idx_f = D.idx_f;
            P.perm_t = D.perm_t;
            P.idx_t = D.idx_t;
            P.row0 = c->rows.row0.as<int32_t>();
            P.zero_row = (int32_t)c->rows.R;
            P.nf = (int32_t)nf;
            P.nt = (int32_t)nt;
            P.tf_list = D.tf_list;
            P.lo = A.lo;
            if (int rc = launch_gemm_lo_units(c, P, mixed->n_tf, c->stream)) return rc;
        }
        launch_units(A, D, U, ghist, c->stream);
        LDW_HIP(hipGetLastError());
    } else {
        // the straight-line units first (k_mi_epilogue_fast: 5 waves per SIMD), then the predicated code over the units it listed (ldw_mi_eval.inc)
        // (read per call: A/B, and the test runs both forms; the fast kernel reads int64 sums of the full weights: what this branch always has)
        const bool split = getenv("LDW_NO_EPI_SPLIT") == nullptr && !A.E.apx && !A.lo.on;
        if (split) {
            if (int rc = c->epi_rest.reserve((size_t)egrid.x * (size_t)nt * 8 + 64)) return rc;   // (worst case: every unit of the block)
            unsigned int *n_rest = c->epi_rest.as<unsigned int>();
            uint64_t *rest = reinterpret_cast<uint64_t *>(c->epi_rest.as<char>() + 64);
            LDW_HIP(hipMemsetAsync(n_rest, 0, 64, c->stream));
            const int mode = !A.E.cols ? 0 : (A.E.spec_B >= 0 ? 2 : 1);
            with_rxy_mode(rxy_read_mode(quirk, A.span, nf == nt), [&](auto RM) {
                constexpr int rm = decltype(RM)::value;
                if (mode == 0) hipLaunchKernelGGL((k_mi_epilogue_fast<rm, 0>), egrid, dim3(256), 0, c->stream, A, D.perm, D.perm_t, ghist, rest, n_rest);
                else if (mode == 1) hipLaunchKernelGGL((k_mi_epilogue_fast<rm, 1>), egrid, dim3(256), 0, c->stream, A, D.perm, D.perm_t, ghist, rest, n_rest);
                else hipLaunchKernelGGL((k_mi_epilogue_fast<rm, 2>), egrid, dim3(256), 0, c->stream, A, D.perm, D.perm_t, ghist, rest, n_rest);
            });
            LDW_HIP(hipGetLastError());
            hipLaunchKernelGGL(k_mi_epilogue_rest, dim3(1024), dim3(256), 0, c->stream, A, D.perm, D.perm_t, ghist, (const uint64_t *)rest, (const unsigned int *)n_rest);
        } else {
            hipLaunchKernelGGL(k_mi_epilogue, egrid, dim3(256), 0, c->stream, A, D.perm, D.perm_t, ghist);
        }
        LDW_HIP(hipGetLastError());
    }
    LDW_HIP(hipEventRecord(ev[2], c->stream));
    return LDW_OK;
}

// ------------------------------------------------------------------------------------------------
// One block in the approximate-GEMM path (ldw_apx.h), in two phases so that the block-wide work of block b+1 runs beside
// the tail of block b:
//   phase 1 (stream gs): pack the bit panels of both row lists, the dual-digit int8 pass into the int32 block (not for an
//            SR-only pass: it screens without MI), per-block SNP constants, the approximate screens -> unit lists (units
//            that hold a short-range pair) and pair lists (the other long-range candidates), and the EXACT 5-limb GEMM of
//            the tiles that hold a short-range pair (band_mask: the short-range band is dense, a fifth of a diagonal block);
//   phase 2 (main stream): exact sums + fp64 MI + emission of the listed pairs (k_pair_sums, k_pair_mi) and the fp64
//            evaluation of the listed units from the exact tiles (k_mi_units).
// Everything phase 1 writes is per pipeline slot; both phases take their pointers from ONE description of each of the slot's buffers (ldw_slots.h).
// Events: ev[0] / ev[1] around the packing + approximate GEMM, ev[5] after the screens and the band GEMM (gs); ev[4] / ev[2]
// around phase 2.
// ------------------------------------------------------------------------------------------------
int launch_block_apx(ldw_ctx *c, const DevPtrs &D, int64_t nf, int64_t nt, int RFpad, int RTpad, int quirk, EmitArgs E, const hipEvent_t *ev, int phase,
                     hipStream_t gs, unsigned long long *ghist, const LoHost *lo_h, void *zero_hist = nullptr, void *zero_pick = nullptr,
                     size_t zero_pick_bytes = 0) {
    const int s = lo_h->slot;
    hipStream_t s2 = c->stream;   // stream of phase 2
    E.nf = (int)nf;
    E.MI = nullptr;
    dim3 egrid((unsigned)(D.nf_tiles > 0 ? D.nf_tiles : (nf + 63) / 64), (unsigned)((nt + EPI_COLS - 1) / EPI_COLS));
    LDW_REQUIRE(egrid.y <= 65535u, LDW_ERR_ARG, "nt too large for the epilogue grid");
    LDW_REQUIRE(E.scr_mode && E.cols && !E.write_dense, LDW_ERR_STATE, "the approximate path needs the screen");
    // the slot's buffers: phase 1 reserves them, phase 2 finds them where phase 1 left them
    const SlotGeom g{nf, nt, RFpad, RTpad, (int64_t)egrid.x, lo_h->span, false};
    UnitsLayout U(g);
    PacksLayout K(g);
    BinsLayout B(g);
    MiniLayout M(g);
    const uint32_t pl_cap = pair_cap_for(nf, nt, lo_h->span), maybe_cap = maybe_cap_for(RTpad, RFpad);
    PairsLayout PL(pl_cap, maybe_cap);
    auto place = [c, phase](Carve &cv, ldw::DevBuf &b) {
        if (phase == 1) {
            c->cnt.slot_grown += cv.bytes > b.cap || !b.p ? 1 : 0;
            return cv.reserve(b);
        }
        cv.bind(b);
        return (int)LDW_OK;
    };
    const bool use_pairs = E.scr_mode == 1 && E.do_lr;   // verify mode keeps whole units: it must see the dismissed ones
    // units are evaluated from EXACT sums: the 5-limb GEMM of the tiles they live in (all tiles when any unit can be listed)
    const bool need_exact = E.any_sr || !use_pairs || lo_h->band_full;
    const uint8_t *band = (use_pairs && !lo_h->band_full) ? D.band_mask : nullptr;
    // r04: the exact band GEMM in phase 1, on the GEMM stream — for alignments of at least 4096 sequences, where the GEMMs are long: see
    // screen_main below
    const int64_t swap_kw = [] { const char *e = getenv("LDW_QUEUE_SWAP_KW"); return e ? (int64_t)atol(e) : (int64_t)64; }();   // (per call: the tests lower it)
    const bool band_early = c->KW >= swap_kw;
    ldw::DevBuf &Gx = gx(c, s);
    if (phase == 1) {
        if (int rc = c->panel[s][0].reserve((size_t)RFpad * c->KW * 16)) return rc;   // (the scaled panel of k_pack_panel: 16 bytes per word)
        if (!lo_h->diag)
            if (int rc = c->panel[s][1].reserve((size_t)RTpad * c->KW * 16)) return rc;
        if (E.do_lr)
            if (int rc = c->Gapx[s].reserve((size_t)RFpad * RTpad * 4)) return rc;
        if (need_exact)
            if (int rc = Gx.reserve((size_t)RFpad * RTpad * 8)) return rc;
        if (int rc = c->apx_clean[s].reserve((size_t)(RTpad / 32) * (size_t)(RFpad / 64) + 64)) return rc;
        if (!c->apx_skip.p) {
            if (int rc = c->apx_skip.reserve(64)) return rc;
            LDW_HIP(hipMemsetAsync(c->apx_skip.p, 0, 64, gs));
        }
    }
    if (int rc = place(U, c->apx_units[s])) return rc;
    if (int rc = place(K, c->apx_packs[s])) return rc;
    if (int rc = place(B, c->apx_bins[s])) return rc;
    if (use_pairs)
        if (int rc = place(PL, c->pairs[s])) return rc;
    if (phase == 1) {
        if (E.do_lr) {
            // threshold table of the biallelic pairs, one per block kind (diagonal blocks sit ~8 % below the others): valid for every
            // block whose level is at least the level it was built for — a higher level only widens the true interval, i.e. the
            // table gets looser, and how tight it is decides how many regions the GEMM's epilogue finds clean — so it is rebuilt as
            // soon as the block's level has left [tab_lo, 1.05 tab_lo] (one bucket = 0.5 %).  Phase 1 of every block runs in order
            // on ONE stream, so the rebuild cannot overtake a reader.
            const int kd = lo_h->diag ? 1 : 0;
            const double lo_blk = E.spec_lo - (double)E.scr_eps;
            if (!(c->spec.tab11_lo[kd] > 0) || lo_blk < c->spec.tab11_lo[kd] || lo_blk > 1.05 * c->spec.tab11_lo[kd]) {
                constexpr int NBINS_T = 64;
                if (int rc = c->spec.tab11[kd].reserve((size_t)4 * NBINS_T * NBINS_T * 8)) return rc;   // a ring of four tables
                c->spec.tab11_cur[kd] = (c->spec.tab11_cur[kd] + 1) & 3;   // (items in flight — at most the two before this one — keep the tables they were screened for)
                const double W = std::ldexp((double)c->wts.total_fixed, -c->wts.frac_bits);
                c->spec.tab11_lo[kd] = 0.98 * lo_blk;   // buckets are 0.5 % wide: the next blocks of the kind may guess four buckets lower (six higher) without a rebuild (73 us)
                c->spec.tab11_c = (float)(NBINS_T / std::sqrt(W + 1.0));
                c->spec.tab11_nb = NBINS_T;
                const double sprime = std::ldexp(1.0, c->apx.apx_e_last - c->wts.frac_bits);
                hipLaunchKernelGGL(k_build_tab11, dim3(NBINS_T * NBINS_T * 32 / 256), dim3(256), 0, gs, W, c->spec.tab11_lo[kd], c->apx.apx_delta * 1.001,
                                   (c->apx.apx_lost_units + 1.0) * sprime, sprime, NBINS_T, c->spec.tab11_c, c->spec.tab11[kd].as<int2>() + (size_t)c->spec.tab11_cur[kd] * NBINS_T * NBINS_T);
                LDW_HIP(hipGetLastError());
                ++c->cnt.tab11_builds;
            }
        }
    }
    EpiArgs A;
    fill_epi_args(c, D, nf, nt, RFpad, quirk, E, reinterpret_cast<const int64_t *>(c->Gapx[s].p), A);
    A.lo.slot_pfix_hi = c->rows.slot_papx.as<int64_t>();   // the screen derives its cells from the marginals of the approximate weights
    if (lo_h->span) {
        LDW_REQUIRE(E.scr_mode == 1 && E.do_lr && !E.any_sr && !lo_h->band_full && lo_h->fuse_ok && lo_h->sseg, LDW_ERR_STATE, "a span needs long-range-only blocks and pair lists");
        A.span = lo_h->span;
        for (int k = 0; k < lo_h->span; ++k) A.sseg[k] = lo_h->sseg[k];
    }
    const int kd_tab = lo_h->diag ? 1 : 0;
    // (the table is built for RXY = 1, the floor of the reference's scrambled RXY = r r' / 4 as long as no SNP has r < 2)
    if (phase == 1 || !lo_h->tab_set) {
        lo_h->tab_p = nullptr;
        if (E.do_lr && c->spec.tab11[kd_tab].p && c->spec.tab11_lo[kd_tab] > 0 && E.spec_lo - (double)E.scr_eps >= c->spec.tab11_lo[kd_tab] &&
            (quirk != LDW_QUIRK_REFERENCE || c->meta.r_min >= 2.0))
            lo_h->tab_p = c->spec.tab11[kd_tab].as<int2>() + (size_t)c->spec.tab11_cur[kd_tab] * 64 * 64;
        lo_h->tab_set = true;
    }
    if (lo_h->tab_p) {   // (phase 2: the table of phase 1, whatever later items have built since)
        A.tab11 = lo_h->tab_p;
        A.tab_nb = c->spec.tab11_nb;
        A.tab_c = c->spec.tab11_c;
    }
    // long-range-only blocks: the GEMM applies the table itself and neither stores nor lets the screen read the regions that pass
    const bool fuse = lo_h->fuse_ok && A.tab11 && A.tab_nb == 64 && (use_pairs || c->knobs.screen == 2) && E.do_lr && (!E.any_sr || (D.band_mask && !lo_h->band_full)) && RFpad % 64 == 0 &&   // (verify mode: the clean regions' units are listed as dismissed and checked in fp64)
                      2048 + (size_t)(c->KW / 2) * 256 + 64 * 64 * 8 + 1024 <= 65536;   // (the table shares the GEMM's LDS with the digit arrays)
    // pruning flags by row and by epilogue slot
    const bool wide_prune = c->knobs.prune && c->rows.snp_sup.p && E.do_lr && (use_pairs || c->knobs.screen == 2);
    uint8_t *sflag_f = nullptr, *sflag_t = nullptr, *rflag_f = nullptr, *rflag_t = nullptr;
    if (wide_prune) {
        sflag_f = B.sflag_f;
        sflag_t = B.sflag_t;
        rflag_f = B.rflag_f;
        rflag_t = B.rflag_t;
        A.snp_sup = c->rows.snp_sup.as<double>();
        A.sflag_f = sflag_f;
        A.sflag_t = sflag_t;
    }
    if (fuse) {
        A.clean = c->apx_clean[s].as<uint8_t>();
        A.clean_stride = RFpad / 64;
    }
    if (use_pairs) {
        A.pl_n = PL.hdr;
        A.pl_pairs = PL.lists;
        A.pl_cap = pl_cap;
    }
    // r04: table-eligible regions with a few failing entries hand those entries over instead of being stored and screened (k_screen_maybe);
    // the counter lives in the zeroed header of the pair lists, the entries behind the lists
    const bool maybe_on = getenv("LDW_NO_MAYBE") == nullptr;   // (read per call: the tests switch it)
    // (only where the K loop is long enough to carry the epilogue's extra work — the mask of the failing entries is built for every eligible
    // region: at N = 616 the GEMM's launch went from 0.091 to 0.107 ms and the pass from 19.4 to 20.1 ms with it, at N = 5000 the launch does
    // not move and the pass gains 0.3-0.4 ms; building the mask only in failing regions was slower at both sizes)
    const bool use_maybe = maybe_on && !c->spec.maybe_off && fuse && use_pairs && c->knobs.screen == 1 && !E.lower_only && c->KW >= 32;
    unsigned int *maybe_n = nullptr;
    ApxMaybe *maybe_list = nullptr;
    MiniCol *mini_c = nullptr;
    MiniRow *mini_r = nullptr;
    if (use_maybe) {
        maybe_n = PL.hdr + PH_MAYBE_N;
        maybe_list = PL.maybe;
        if (int rc = place(M, c->apx_mini[s])) return rc;
        A.mini_c = mini_c = M.col;
        A.mini_r = mini_r = M.row;
    }
    if (phase == 1) {
        if (E.do_lr) {
            if (int rc = launch_pack_panel(c, D.rl_f, RFpad, c->panel[s][0].as<uint64_t>(), gs, lo_h->diag ? nullptr : D.rl_t, RTpad,
                                           lo_h->diag ? nullptr : c->panel[s][1].as<uint64_t>()))
                return rc;
        }
        {   // the unit counters, the pair-list counters, this slot's histogram and pick record (submit_b skips its own memsets)
            ZeroArgs Z;
            memset(&Z, 0, sizeof(Z));
            auto zero = [&Z](int k, const Carve::Range &r) {
                Z.p[k] = reinterpret_cast<uint4 *>(r.p);
                Z.n16[k] = r.n16();
            };
            zero(0, U.zeroed());
            if (use_pairs) zero(1, PL.zeroed());
            if (fuse) {
                // Every region must read "not clean" unless THIS block's GEMM (or its live-tile pass) says otherwise.  r01-r05 zeroed the flags of diagonal
                // blocks only (the GEMM skips their tiles above the diagonal) and relied on every other region being rewritten by every launch — which holds
                // block after block of one shape, but tools/fuzz_paths.py (r05) found flags of an EARLIER, larger problem read by a later one on the same
                // context (N = 40 after N = 257: 334 pairs the screen would have lost in verify mode).  66 KB per 10k x 10k block, in the memset the slot gets anyway.
                Z.p[4] = reinterpret_cast<uint4 *>(c->apx_clean[s].p);
                Z.n16[4] = (unsigned int)(((size_t)(RTpad / 32) * (size_t)(RFpad / 64) + 15) / 16);
            }
            zero(5, B.zeroed());
            if (zero_hist) {
                Z.p[2] = reinterpret_cast<uint4 *>(zero_hist);
                Z.n16[2] = (unsigned int)((size_t)NBINS * 8 / 16 * (size_t)(lo_h->span ? lo_h->span : 1));   // (a span: one histogram per reference block)
                Z.p[3] = reinterpret_cast<uint4 *>(zero_pick);
                Z.n16[3] = (unsigned int)(zero_pick_bytes / 16);
            }
            hipLaunchKernelGGL(k_zero4, dim3(16), dim3(256), 0, gs, Z);
        }
        // the per-SNP constants in epilogue order — before the GEMM: its epilogue reads the table bins by row
        const int nthr = std::max<int>(std::max<int>((int)nt, (int)g.nf_slots()), std::max<int>(RTpad, RFpad));
        hipLaunchKernelGGL(k_build_packs, dim3((unsigned)((nthr + 255) / 256), 2), dim3(256), 0, gs, A, D.perm, D.perm_t, (int)g.nf_slots(), 1, K.cp, K.cp_hi, K.rp,
                           K.rp_hi, K.rloc_f, K.rloc_t, B.bin_t, B.bin_f, RTpad, RFpad, sflag_f, sflag_t, rflag_f, rflag_t, mini_c, mini_r);
        LDW_HIP(hipGetLastError());
        ApxGemmArgs P;
        if (E.do_lr) {
            memset(&P, 0, sizeof(P));
            P.panel_f = c->panel[s][0].as<uint64_t>();
            P.panel_t = lo_h->diag ? P.panel_f : c->panel[s][1].as<uint64_t>();
            P.RTpad = RTpad;
            P.RFpad = RFpad;
            P.M2 = (int)(c->KW / 2);
            P.dig_a = c->apx.dig_a.as<uint8_t>();
            P.dig_b = c->apx.dig_b.as<uint8_t>();
            P.shift = c->apx.apx_shift.as<int32_t>();
            P.fine = c->apx.apx_fine ? 1 : 0;
            P.G = c->Gapx[s].as<int32_t>();
            P.lower_only = E.lower_only;
            if (fuse) {
                P.fuse = 1;
                P.skip_ctr = (c->knobs.prune && lo_h->ordered) ? c->apx_skip.as<unsigned long long>() : nullptr;   // (list order: a tile spans every bin)
                if (P.skip_ctr) {
                    P.tile_list = B.tile_list;
                    P.n_live = B.n_live;
                    P.grid_wgs = apx_run_grid(c, RTpad, RFpad);   // every wave walks a run of the list
                    P.rflag_t = rflag_t;
                    P.rflag_f = rflag_f;
                }
                P.bin_t = B.bin_t;
                P.bin_f = B.bin_f;
                P.tab = A.tab11;
                P.tab_nb = A.tab_nb;
                P.clean = c->apx_clean[s].as<uint8_t>();
                P.sr_mask = E.any_sr ? D.band_mask : nullptr;   // a block with a short-range corner: its band tiles stay with the screen
                if (use_maybe) {
                    P.maybe = maybe_list;
                    P.maybe_n = maybe_n;
                    P.maybe_cap = maybe_cap;
                }
            }
            if (P.skip_ctr)
                if (int rc = launch_apx_live_tiles(c, P, gs)) return rc;
        }
        LDW_HIP(hipEventRecord(ev[0], gs));   // ev[0] .. ev[1]: the approximate GEMM alone (its launch time is the roofline's)
        if (E.do_lr)
            if (int rc = launch_gemm_apx(c, P, gs)) return rc;
        LDW_HIP(hipEventRecord(ev[1], gs));
    }
    bind_packs(A, K, true);
    // The block's screen at the head of phase 2 on the main stream — beside the NEXT block's GEMM on the GEMM stream — instead of behind
    // its own GEMM.
    // (r04, first attempt: a span's screen at the head of phase 2 went WRONG — phase 2 is queued after the first phase of LATER items, which may
    // rebuild the threshold table for their level; the screen then either found no table it might use and, with it, no clean flags — it read the
    // regions the GEMM's epilogue had not stored: 20-60 million pairs listed per span at C5, overflowing lists, 43 segments redone per pass — or
    // raced the rebuild.  Cured by LoHost::tab_p: every item keeps the table its first phase chose, out of a ring of four per kind.)
    // r04 (end of the round): with the table a per-item snapshot out of a ring (above) the screen may run at the head of phase 2 on the main
    // stream for every item, and the exact band GEMM moves the other way, into phase 1 on the GEMM stream: one queue holds the MFMA kernels, the
    // other the VALU- and latency-bound ones, which share the CUs better than two GEMMs do (C4, alternating runs: 33.6 / 33.2 against 34.2 / 34.2
    // ms; the band GEMM alone on the GEMM stream: 35.3 / 34.9; three more alternating pairs at the end: 33.6 / 33.2 / 33.4 against 34.0 / 33.8 /
    // 34.0; C5 819 against 824 ms, 3 misses per pass either way).  Only where the GEMMs are long (N >= 4096): at 85k x 616 the approximate GEMM
    // is 2.7 ms of a 19-ms pass, the GEMM queue would idle and the main queue carry everything — 20.9 / 21.1 against 19.3 / 19.1 ms — so short
    // alignments keep the old places.
    const bool screen_main = c->KW >= swap_kw;
    const int rm = rxy_read_mode(quirk, lo_h->span, nf == nt);
    auto screen = [&](hipStream_t st) {
        with_rxy_mode(rm, [&](auto RM) {
            hipLaunchKernelGGL((k_mi_screen<decltype(RM)::value, true>), egrid, dim3(256), 0, st, A, D.perm, D.perm_t, U.flat, U.counters, U.list_stride);
        });
    };
    if (phase == 1) {
        if (!screen_main) {
            screen(gs);
            LDW_HIP(hipGetLastError());
        }
        if (band_early && need_exact)
            if (int rc = launch_gemm_bits(c, c->rows.Mbits.as<uint64_t>(), c->KW, D.rl_t, RTpad, D.rl_f, RFpad, Gx.as<int64_t>(), c->wts.nlimbs, c->wts.digits.as<int8_t>(),
                                          E.lower_only, gs, 0, -1, band, band ? D.band_list : nullptr, D.n_band))
                return rc;
        if (use_maybe && E.do_lr) {
            constexpr unsigned MAYBE_GRID = 512u;   // (r05: 512 / 2048 / 8192 / 32768 workgroups measured on the adversarial alignment — no difference: the kernel was bound by its atomics)
            with_rxy_mode(rm, [&](auto RM) {
                hipLaunchKernelGGL((k_screen_maybe<decltype(RM)::value>), dim3(MAYBE_GRID), dim3(256), 0, gs, A, maybe_list, maybe_n, maybe_cap);
            });
            LDW_HIP(hipGetLastError());
        }
        LDW_HIP(hipEventRecord(ev[5], gs));
        return LDW_OK;
    }
    // ---- phase 2 ----
    LDW_HIP(hipEventRecord(ev[4], s2));
    if (screen_main) {
        screen(s2);
        LDW_HIP(hipGetLastError());
    }
    launch_screen_generic<true>(A, D, (int)egrid.x, U, s2);
    LDW_HIP(hipGetLastError());
    if (need_exact && !band_early)
        if (int rc = launch_gemm_bits(c, c->rows.Mbits.as<uint64_t>(), c->KW, D.rl_t, RTpad, D.rl_f, RFpad, Gx.as<int64_t>(), c->wts.nlimbs, c->wts.digits.as<int8_t>(),
                                      E.lower_only, s2, 0, -1, band, band ? D.band_list : nullptr, D.n_band))
            return rc;
    if (use_pairs) {
        if (int rc = c->pair_sums.reserve((size_t)PAIR_PATHS * PAIR_SHARDS * A.pl_cap * 16 * 8)) return rc;
        if (int rc = launch_pairs_exact(c, A, ghist, c->pair_sums.as<int64_t>(), s2)) return rc;
    }
    if (need_exact) {   // the listed units, from the exact tiles
        EpiArgs Ax = A;
        Ax.G = Gx.as<int64_t>();
        Ax.E.apx = 0;
        Ax.pl_pairs = nullptr;
        launch_units(Ax, D, U, ghist, s2);
    }
    hipLaunchKernelGGL(k_apx_stats, dim3(1), dim3(64), 0, s2, U.counters, A.pl_n, A.pl_cap, A.E.scr_viol + 1);
    LDW_HIP(hipGetLastError());
    LDW_HIP(hipEventRecord(ev[2], s2));
    return LDW_OK;
}

// lane order of the epilogue: from-side SNPs grouped by their number of indicator rows (1, 2, 3, 4, 0)
// The same for the from side of the epilogue kernels, which walk it in tiles of 64 (one wave): every class is padded
// with -1 to a multiple of 64, so no tile mixes slot counts — a mixed tile cannot take the straight-line code and
// would have all of its units listed for the fp64 kernel (and for the gathered low-limb GEMM).
void build_perm_tiles(ldw_ctx *c, const int32_t *from_idx, int64_t nf, std::vector<int32_t> &perm, const std::vector<int32_t> *order1 = nullptr) {
    perm.clear();
    for (int want : {1, 2, 3, 4, 0}) {
        if (want == 1 && order1) perm.insert(perm.end(), order1->begin(), order1->end());   // (every one-row SNP, in row order: build_side)
        else
            for (int64_t k = 0; k < nf; ++k)
                if (c->rows.h_row0[from_idx[k] + 1] - c->rows.h_row0[from_idx[k]] == want) perm.push_back((int32_t)k);
        if (want != 3)   // 3 and 4 rows share the generic code anyway
            while (perm.size() % 64) perm.push_back(-1);
    }
    if (perm.empty()) perm.assign(64, -1);
}

void build_perm(ldw_ctx *c, const int32_t *from_idx, int64_t nf, int32_t *perm, const std::vector<int32_t> *order1 = nullptr) {
    int64_t w = 0;
    for (int want : {1, 2, 3, 4, 0}) {
        if (want == 1 && order1) {
            for (int32_t k : *order1) perm[w++] = k;
            continue;
        }
        for (int64_t k = 0; k < nf; ++k)
            if (c->rows.h_row0[from_idx[k] + 1] - c->rows.h_row0[from_idx[k]] == want) perm[w++] = (int32_t)k;
    }
}

// The one-row SNPs of a list in ascending order of h_minor_w (ties in list order), cached per list: the all-pairs loop presents
// the same ten or fifty lists over and over, and a sort of 10^4 keys costs as much host time as the rest of prep_block.
// Entries are heap objects and are never removed while the row map lives (ensure_rows clears the cache): the pointers handed out stay
// valid whatever another thread adds; a full cache (256 lists) computes into the caller's own vector instead.
const std::vector<int32_t> *minor_weight_order(ldw_ctx *c, const int32_t *idx, int64_t n, std::vector<int32_t> &own) {
    {
        std::lock_guard<std::mutex> lk(c->rows.order_mtx);
        for (auto &pe : c->rows.order_cache)
            if ((int64_t)pe->idx.size() == n && pe->idx[0] == idx[0] && memcmp(pe->idx.data(), idx, (size_t)n * 4) == 0) return &pe->order;
    }
    std::vector<std::pair<int64_t, int32_t>> key;
    key.reserve((size_t)n);
    for (int64_t k = 0; k < n; ++k)
        if (c->rows.h_row0[idx[k] + 1] - c->rows.h_row0[idx[k]] == 1) key.emplace_back(c->rows.h_minor_w[(size_t)idx[k]], (int32_t)k);
    std::sort(key.begin(), key.end());
    own.resize(key.size());
    for (size_t i = 0; i < key.size(); ++i) own[i] = key[i].second;
    std::lock_guard<std::mutex> lk(c->rows.order_mtx);
    if (c->rows.order_cache.size() >= 256) return &own;
    c->rows.order_cache.emplace_back(new ldw::OrderCache());
    auto &e = *c->rows.order_cache.back();
    e.idx.assign(idx, idx + n);
    e.order = own;
    return &e.order;
}

// dense MI of one block, synchronous staging through ctx-owned buffers (ldw_mi_block, ldw_joint_tables style)
int run_block_mi(ldw_ctx *c, const int32_t *from_idx, int64_t nf, const int32_t *to_idx, int64_t nt, int quirk,
                 EmitArgs E) {
    if (int rc = join_prepare(c)) return rc;
    if (int rc = ensure_rows(c)) return rc;
    LDW_REQUIRE(nf > 0 && nt > 0, LDW_ERR_ARG, "empty block (nf=%lld nt=%lld)", (long long)nf, (long long)nt);
    LDW_REQUIRE(nf <= 1000000 && nt <= 1000000, LDW_ERR_ARG, "block side too long");
    std::vector<int32_t> vf(from_idx, from_idx + nf), vt(to_idx, to_idx + nt), perm, perm_t((size_t)nt);
    SideLists SF, ST;
    if (int rc = build_side(c, from_idx, nf, SF)) return rc;
    if (int rc = build_side(c, to_idx, nt, ST)) return rc;
    build_perm_tiles(c, from_idx, nf, perm);
    build_perm(c, to_idx, nt, perm_t.data());
    if (int rc = upload_i32(c, c->perm_t, perm_t)) return rc;
    if (int rc = upload_i32(c, c->idx_f, vf)) return rc;
    if (int rc = upload_i32(c, c->idx_t, vt)) return rc;
    if (int rc = upload_i32(c, c->rowlist_f, SF.rowlist)) return rc;
    if (int rc = upload_i32(c, c->rowlist_t, ST.rowlist)) return rc;
    if (int rc = upload_i32(c, c->lrow_f, SF.lrow)) return rc;
    if (int rc = upload_i32(c, c->lrow_t, ST.lrow)) return rc;
    if (int rc = upload_i32(c, c->perm_f, perm)) return rc;
    if (int rc = c->hist[0].reserve((size_t)NBINS * 8)) return rc;
    LDW_HIP(hipStreamSynchronize(c->stream));  // pageable H2D copies are complete only after a sync
    DevPtrs D{};   // (no intervals, row positions, classes, low-limb geometry or band: the dense path reads none of them)
    D.idx_f = c->idx_f.as<int32_t>();
    D.idx_t = c->idx_t.as<int32_t>();
    D.rl_f = c->rowlist_f.as<int32_t>();
    D.rl_t = c->rowlist_t.as<int32_t>();
    D.lrow_f = c->lrow_f.as<int32_t>();
    D.lrow_t = c->lrow_t.as<int32_t>();
    D.perm = c->perm_f.as<int32_t>();
    D.perm_t = c->perm_t.as<int32_t>();
    D.nf_tiles = (int)(perm.size() / 64);
    D.gen_t0 = D.gen_q0 = 0x7FFFFFFF;
    E.write_dense = 1;
    E.spec_B = -1;
    // a symmetric block (same list on both sides) may be asked for in full: the GEMM then computes every tile
    return launch_block_mi(c, D, nf, nt, SF.Rpad, ST.Rpad, quirk, E, handles(c->ev), 3, nullptr, nullptr, c->hist[0].as<unsigned long long>());
}

int ensure_links_capacity(ldw_ctx *c, int64_t sr_rows, int64_t lr_rows) {
    // a reallocation (rare: the all-pairs driver sizes the table up front) waits for the GEMM stream and is complete before
    // anything else is queued
    const bool grow_sr = (size_t)sr_rows * 8 > c->links.sr_mi.cap || (size_t)sr_rows * 4 > c->links.sr_a.cap || (size_t)sr_rows * 4 > c->links.sr_b.cap;
    if (grow_sr && c->gemm_stream) LDW_HIP(hipStreamSynchronize(c->gemm_stream));
    if (int rc = c->links.sr_a.reserve_keep((size_t)sr_rows * 4, (size_t)c->links.n_sr * 4, c->stream)) return rc;
    if (int rc = c->links.sr_b.reserve_keep((size_t)sr_rows * 4, (size_t)c->links.n_sr * 4, c->stream)) return rc;
    if (int rc = c->links.sr_mi.reserve_keep((size_t)sr_rows * 8, (size_t)c->links.n_sr * 8, c->stream)) return rc;
    if (grow_sr) LDW_HIP(hipStreamSynchronize(c->stream));
    if (c->lr_stream && ((size_t)lr_rows * 8 > c->links.lr_mi.cap || (size_t)lr_rows * 4 > c->links.lr_a.cap || (size_t)lr_rows * 4 > c->links.lr_b.cap))
        lr_stream_drain(c);   // (the writer thread reads these buffers on its own stream: everything handed over is on disk before they move)
    if (int rc = c->links.lr_a.reserve_keep((size_t)lr_rows * 4, (size_t)c->links.n_lr * 4, c->stream)) return rc;
    if (int rc = c->links.lr_b.reserve_keep((size_t)lr_rows * 4, (size_t)c->links.n_lr * 4, c->stream)) return rc;
    if (int rc = c->links.lr_mi.reserve_keep((size_t)lr_rows * 8, (size_t)c->links.n_lr * 8, c->stream)) return rc;
    return LDW_OK;
}

// layout of ctx->small during link selection
struct SmallLayout {
    int64_t *lr_count;   // running number of kept long-range rows (device side)
    ldw::PickOut *pick[LDW_NSLOT];   // one per pipeline slot
    int64_t *stats_i;    // [capacity][3]
    double *stats_d;     // [capacity]
};

constexpr size_t PICK_STRIDE = ((sizeof(ldw::PickOut) + 63) / 64) * 64;

void links_layout(ldw_ctx *c, SmallLayout &sl) {
    char *base = c->small.as<char>();
    sl.lr_count = reinterpret_cast<int64_t *>(base);
    // (every slot has room for the pick records of a span's segments: segment k of slot s at sl.pick[s] + k * PICK_STRIDE bytes)
    for (int k = 0; k < LDW_NSLOT; ++k) sl.pick[k] = reinterpret_cast<ldw::PickOut *>(base + 64 + (size_t)k * LDW_SPAN_MAX * PICK_STRIDE);
    sl.stats_i = reinterpret_cast<int64_t *>(base + 64 + (size_t)LDW_NSLOT * LDW_SPAN_MAX * PICK_STRIDE);
    sl.stats_d = reinterpret_cast<double *>(sl.stats_i + c->links.blk_capacity * 3);
}


// Part of ldw_mi.hip (inside its anonymous namespace): the ITEM pipeline of the all-pairs loop — HostBlock, prep_block (pure host, run by the
// helper threads), submit_a / submit_b / finish_block / finish_span (the phases of an item), the redo of a span's segment, the cold-start probes.
// ---- one block of the link loop in phases so that the host work and the GEMM of block i+1 overlap the selection of block i:
// ----   prep     pure host, into pinned memory
// ----   submit_a upload, then the GEMM on the GEMM stream
// ----   submit_b epilogue + bucket pick + copy-back on the main stream
// ----   finish   the one host round trip (candidate count), then sorts / threshold / append on the main stream

// The staging image of a block: the index structures of both sides, one behind the other (64-byte aligned: the kernels read them with wide loads) in
// the item's pinned buffer, sent to the device as one copy.  array<&DevPtrs::x>(src, count) names an array ONCE — its element type is that of the
// DevPtrs field, src its host source (null: built in place), count its elements — and from that statement come its offset (returned), its copy into
// the pinned buffer (copy_to) and its typed device pointer (bind, once the device base is known; an array that is not named keeps its null).
// The parts live in the HostBlock and nothing is allocated; src is good until prep_block returns.
struct StageImage {
    struct Part {
        size_t off, bytes;
        const void *src;
        void (*point)(DevPtrs &, const char *);
    };
    Part part[18] = {};   // (the array<> statements of prep_block)
    int n = 0;
    size_t bytes = 0;     // of the whole image
    template <class T> static T elem_of(const T *DevPtrs::*);
    template <auto F> using Elem = decltype(elem_of(F));
    template <auto F> size_t array(const Elem<F> *src, size_t count) {
        part[n] = Part{bytes, count * sizeof(Elem<F>), src, [](DevPtrs &D, const char *p) { D.*F = reinterpret_cast<const Elem<F> *>(p); }};
        bytes = (bytes + part[n].bytes + 63) / 64 * 64;
        return part[n++].off;
    }
    void copy_to(char *image) const {
        for (int k = 0; k < n; ++k)
            if (part[k].src && part[k].bytes) memcpy(image + part[k].off, part[k].src, part[k].bytes);
    }
    void bind(DevPtrs &D, const char *image) const {
        for (int k = 0; k < n; ++k) part[k].point(D, image + part[k].off);
    }
};

struct HostBlock {
    int64_t nf = 0, nt = 0, n_sr_blk = 0, n_lr_total = 0, blk_no = 0;
    int RFpad = 0, RTpad = 0, slot = 0;
    bool diag = false, submitted = false;
    bool uploaded = false;     // submit_upload has queued the upload of its lists (submit_a then skips it)
    bool mixed = false;        // high-limb GEMM + gathered low limbs (decided with the bucket guess at submit_a)
    bool apx = false;          // approximate GEMM + exact popcount sums of the listed units (ldw_apx.h); implies the lo geometry
    bool generic = false;      // a SNP list of the block is not ascending in POS: plain path + the k_gen_* pair list
    int guess = -1;            // bucket guess the block was submitted with
    LoHost lo;
    StageImage img;            // where each array sits in the staging image, and the image's bytes
    size_t total = 0;
    DevPtrs D{};               // prep_block sets the counts, fill_dev_ptrs the pointers
    EmitArgs E{};
    int spec_B = -1;
    // r04 span (ldw_epi.h): the to side is the concatenation of `span` reference blocks (0: an ordinary block)
    int span = 0;
    int32_t seg_start[LDW_SPAN_MAX] = {}, seg_nt[LDW_SPAN_MAX] = {};
    int64_t seg_lr_total[LDW_SPAN_MAX] = {};
    size_t cand_cap = 0;               // entries of every segment's candidate list
    SpanSeg sseg[LDW_SPAN_MAX] = {};
    int pin_slot = -1;                 // staging buffer the lists were built in (-1: the slot's own)
    bool force_plain = false;          // never speculate: a span's segment that is redone after a wrong guess
    bool span_alone = false;           // the span could not be submitted as one (no positive guess): its blocks run one by one in finish_span
    size_t stage_base = 0;             // offset of its image in the staging buffer
    int64_t sr_base = 0;               // first row of the item's short-range rows (set when the item is submitted: submit order = block order)
    std::vector<int32_t> span_from, span_to;   // the span's SNP lists (host): what a segment that runs on its own is prepared from
};

// the to side of a span: where each reference block starts in the concatenated list
struct SpanPlan {
    int nseg = 0;
    int32_t start[LDW_SPAN_MAX] = {}, nt[LDW_SPAN_MAX] = {};
};

// The speculative selection (bucket guess -> approximate GEMM / screen -> lists of the pairs that may pass) pays when the long-range filter
// keeps a small fraction of the pairs.  When lr_retain_links is a sizeable part of lr_links_approx — a small alignment with the default
// 1e6: 5000 SNPs keep 8 % — nearly every unit has to be listed and the lists cost more than evaluating everything: measured on 30k x 2k
// (tools/keep_frac_probe.py, warm passes, default against plain): 6.5 / 11.2 ms at 0.02 %, 21.2 / 21.6 at 0.5 %, 24.1 / 22.8 at 1 %, 84.7 / 24.9 at
// 5 %.  Above 0.7 % every block takes the plain path (5-limb GEMM, fp64 MI of every pair, full histogram), cold start included.
// Only the automatic choice is gated: ldw_set_path(1 | 2) is honoured as given.
static inline bool speculation_pays(const ldw_ctx *c, const ldw_mi_params *p) {
    if (c->knobs.path_mode != 0) return true;
    return !(p->lr_links_approx > 0.0) || p->lr_retain_links < 0.007 * p->lr_links_approx;
}

// One call of prep_block: its lists, and what its stages hand to each other.  A diagonal block's intervals are built by a thread of their own
// (intervals) that writes cols, cols_err and hb.n_sr_blk: join_cols waits for it in front of their first reader, and the destructor before any
// of them goes away, by whichever return prep_block is left.
struct PrepWork {
    ldw_ctx *c;
    const int32_t *from_idx, *to_idx;
    int64_t nf, nt;
    HostBlock &hb;
    std::vector<ColInfo> cols;
    std::string cols_err;
    std::future<int> cols_job;
    const std::vector<int32_t> *ord_f = nullptr, *ord_t = nullptr;        // row order of the one-row SNPs of either side (null: list order)
    std::vector<int32_t> ord_f_own, ord_t_own, ord_f_full, ord_t_full;    // what they point to, unless it is minor_weight_order's cache
    SideLists SF, ST;
    std::vector<int32_t> pf, cmax, tf;   // from-side tiles; widest row-slot class per from-tile; (tile, fs) pairs of the gathered GEMM's grid
    std::vector<int64_t> tbase;          // low-limb block offset per from-tile
    std::vector<uint8_t> band;
    std::vector<uint32_t> bandl;
    // the stages, in the words of the [ldw prep us] line
    int intervals(const ldw_mi_params *p, const SpanPlan *sp);   // hb.generic, cols, hb.n_sr_blk; a span: hb.span / seg_*
    int row_order(const SpanPlan *sp);                           // ord_f / ord_t
    void tiles(int slot);                                        // pf, the counts of hb.D, the low-limb geometry hb.lo, cmax / tbase / tf
    void band_mask();                                            // band, hb.lo.band_full / fuse_ok / ordered (BOUNDS.md)
    bool band_list();                                            // bandl, hb.D.n_band; false: no list, the mask alone
    int join_cols() {
        const int rc = cols_job.valid() ? cols_job.get() : LDW_OK;
        if (rc != LDW_OK) set_error("%s", cols_err.c_str());
        return rc;
    }
    ~PrepWork() { if (cols_job.valid()) cols_job.wait(); }
};

int PrepWork::intervals(const ldw_mi_params *p, const SpanPlan *sp) {
    const int64_t blk_no = hb.blk_no;
    auto ascending = [&](const int32_t *idx, int64_t n) {
        for (int64_t k = 1; k < n; ++k)
            if (c->meta.h_POS[idx[k]] < c->meta.h_POS[idx[k - 1]]) return false;
        return true;
    };
    hb.generic = !ascending(from_idx, nf) || !ascending(to_idx, nt);
    if (hb.generic) {   // no intervals: the pair list is made from the dense block with the predicate itself (submit_b)
        ColInfo z;
        memset(&z, 0, sizeof(z));
        cols.assign((size_t)nt, z);
        hb.n_sr_blk = 0;
    } else if (sp) {
        // a span: the intervals segment by segment (every segment is long-range-only: build_cols leaves at its range test)
        cols.resize((size_t)nt);
        std::vector<ColInfo> ck;
        for (int k = 0; k < sp->nseg; ++k) {
            int64_t n_k = 0;
            if (int rc = build_cols(c, from_idx, nf, to_idx + sp->start[k], sp->nt[k], false, p->sr_dist, ck, n_k)) return rc;
            std::copy(ck.begin(), ck.end(), cols.begin() + sp->start[k]);
        }
        hb.n_sr_blk = 0;
    } else if (hb.diag) {
        // A diagonal block is the first item of a pass — the GPU has nothing to do until its lists are there — and neither its row lists nor
        // its tiles depend on the intervals (no row ordering on the diagonal): the intervals are built on a thread of their own beside them
        // and joined in front of the band, their first reader (0.36 of 1.1 ms at 10k x 10k).
        cols.resize((size_t)nt);
        const double sr_dist = p->sr_dist;
        cols_job = std::async(std::launch::async, [this, sr_dist]() -> int {
            const int rc = build_cols(c, from_idx, nf, to_idx, nt, true, sr_dist, cols, hb.n_sr_blk);
            if (rc != LDW_OK) cols_err = ldw_last_error();
            return rc;
        });
    } else if (int rc = build_cols(c, from_idx, nf, to_idx, nt, hb.diag, p->sr_dist, cols, hb.n_sr_blk)) return rc;
    if (sp) {   // a span: every column learns its reference block and where that block starts in the concatenated to side
        LDW_REQUIRE(!hb.generic && !hb.diag && sp->nseg >= 1 && sp->nseg <= LDW_SPAN_MAX, LDW_ERR_STATE,
                    "span of %d blocks at block %lld cannot be formed", sp->nseg, (long long)blk_no);
        hb.span = sp->nseg;
        for (int k = 0; k < sp->nseg; ++k) {
            hb.seg_start[k] = sp->start[k];
            hb.seg_nt[k] = sp->nt[k];
            hb.seg_lr_total[k] = nf * (int64_t)sp->nt[k] - std::min<int64_t>(nf, sp->nt[k]);   // (off-diagonal blocks drop their own diagonal: Q3)
            for (int32_t b = sp->start[k]; b < sp->start[k] + sp->nt[k]; ++b) {
                cols[(size_t)b].pad[0] = k;
                cols[(size_t)b].pad[1] = sp->start[k];
            }
        }
    }
    return LDW_OK;
}

// Blocks without a short-range pair (most off-diagonal ones): nothing depends on the order of the rows within a class, so the
// one-row SNPs are ordered by the weight of their minor state on both sides — rows and epilogue slots alike, which the table
// test of the GEMM's epilogue requires anyway.  The wave tiles of the approximate GEMM then span few bins of the threshold
// table and the tiles of the rare x rare corner are pruned whole (apx_tile_prunable).
// An off-diagonal block WITH a short-range corner (neighbouring blocks, and the pair that closes the circle): the SNPs that have a
// short-range partner in the block are a few hundred at the facing ends of the two lists.  They keep the list order — the band
// of tiles the exact GEMM covers needs their partners contiguous — behind the ordered rest.  Diagonal blocks stay as they are:
// every SNP has short-range partners there.
int PrepWork::row_order(const SpanPlan *sp) {
    if (c->knobs.prune && !hb.generic && !hb.diag && c->knobs.engine == LDW_ENGINE_MFMA && c->apx.apx_ok) {
        bool rowless = false;
        for (int64_t k = 0; k < nf && !rowless; ++k) rowless = c->rows.h_row0[from_idx[k] + 1] == c->rows.h_row0[from_idx[k]];
        for (int64_t k = 0; k < nt && !rowless; ++k) rowless = c->rows.h_row0[to_idx[k] + 1] == c->rows.h_row0[to_idx[k]];
        if (!rowless) {
            ord_f = minor_weight_order(c, from_idx, nf, ord_f_full);
            ord_t = minor_weight_order(c, to_idx, nt, ord_t_full);
            if (hb.n_sr_blk > 0) {
                std::vector<int32_t> df((size_t)nf + 1, 0);
                std::vector<uint8_t> in_f((size_t)nf, 0), in_t((size_t)nt, 0);
                for (int64_t b = 0; b < nt; ++b)
                    for (int iv = 0; iv < 3; ++iv) {
                        const ColInfo &ci = cols[(size_t)b];
                        if (ci.e[iv] <= ci.s[iv]) continue;
                        in_t[(size_t)b] = 1;
                        ++df[(size_t)ci.s[iv]];
                        --df[(size_t)ci.e[iv]];
                    }
                int32_t run = 0;
                for (int64_t a = 0; a < nf; ++a) {
                    run += df[(size_t)a];
                    in_f[(size_t)a] = run > 0 ? 1 : 0;
                }
                auto rest_then_corner = [&](const std::vector<int32_t> &sorted, const std::vector<uint8_t> &corner, const int32_t *idx, int64_t n,
                                            std::vector<int32_t> &out) {
                    out.clear();
                    out.reserve(sorted.size());
                    for (int32_t k : sorted)
                        if (!corner[(size_t)k]) out.push_back(k);
                    for (int64_t k = 0; k < n; ++k)
                        if (corner[(size_t)k] && c->rows.h_row0[idx[k] + 1] - c->rows.h_row0[idx[k]] == 1) out.push_back((int32_t)k);
                };
                rest_then_corner(*ord_f, in_f, from_idx, nf, ord_f_own);
                rest_then_corner(*ord_t, in_t, to_idx, nt, ord_t_own);
                ord_f = &ord_f_own;
                ord_t = &ord_t_own;
            }
            c->cnt.sorted_blocks += sp ? sp->nseg : 1;
        }
    }
    LDW_REQUIRE(!sp || (ord_f && ord_t), LDW_ERR_STATE, "span at block %lld cannot be ordered", (long long)hb.blk_no);
    return LDW_OK;
}

void PrepWork::tiles(int slot) {
    build_perm_tiles(c, from_idx, nf, pf, ord_f);
    hb.D.nf_tiles = (int)(pf.size() / 64);
    {   // where the SNPs with 1 or 2 indicator rows end in either order
        int64_t n12f = 0, n1 = 0, n2 = 0;
        for (int64_t k = 0; k < nf; ++k) {
            const int nr = c->rows.h_row0[from_idx[k] + 1] - c->rows.h_row0[from_idx[k]];
            n1 += nr == 1;
            n2 += nr == 2;
        }
        n12f = (n1 + 63) / 64 + (n2 + 63) / 64;   // build_perm_tiles pads each of the two classes to whole tiles
        hb.D.gen_t0 = (int)n12f;
        int64_t q12 = 0;
        for (int64_t k = 0; k < nt; ++k) {
            const int nr = c->rows.h_row0[to_idx[k] + 1] - c->rows.h_row0[to_idx[k]];
            q12 += nr == 1 || nr == 2;
        }
        hb.D.gen_q0 = (int)q12;
    }
    // mixed-precision path: row-slot classes of the to side, widest class per from-tile, low-limb block offsets
    // (lo_layout, ldw_lo_geom.h: cmax, tbase and tf — last tiles first — come with it)
    {
        const std::vector<int32_t> &row0 = c->rows.h_row0;
        const LoLayout g = lo_layout(
            nt, [&](int64_t k) { return (int)(row0[to_idx[k] + 1] - row0[to_idx[k]]); }, pf.size(),
            [&](size_t t) { return pf[t] < 0 ? -1 : (int)(row0[from_idx[pf[t]] + 1] - row0[from_idx[pf[t]]]); }, cmax, tbase, tf);
        LoHost &lo = hb.lo;
        lo = LoHost();
        for (int lc = 0; lc < 3; ++lc) {
            lo.n_lc[lc] = g.n_lc[lc];
            lo.uoff[lc] = g.uoff[lc];
            lo.rowbase[lc] = g.rowbase[lc];
            lo.n_tiles_cf[lc] = g.n_tiles_cf[lc];
        }
        lo.RTlo = g.RTlo;
        lo.ntiles = g.ntiles;
        lo.n_tf = g.n_tf;
        lo.glo_total = g.glo_total;
        lo.slot = slot;
        lo.diag = hb.diag ? 1 : 0;
    }
}

// approximate path: tiles of the exact GEMM (128 to-side x 64 from-side rows) that hold a short-range pair.  POS ascends along
// both lists and the row lists keep the list order within a slot-count class, so the partners of a to-side SNP are a
// contiguous row range per class
void PrepWork::band_mask() {
    band.assign((size_t)(hb.RTpad / TILE) * (hb.RFpad / 64), 0);
    bool no_rowless = true;   // no SNP without an indicator row: a one-row SNP's row-list position is its slot (ApxGemmArgs::fuse)
    {
        const int ntx = hb.RFpad / 64;
        auto cls_of = [&](int32_t snp) { const int nr = c->rows.h_row0[snp + 1] - c->rows.h_row0[snp]; return nr <= 1 ? 0 : (nr == 2 ? 1 : 2); };
        std::vector<int32_t> pre[3];
        int32_t base[3] = {0, 0, 0};
        for (int k = 0; k < 3; ++k) pre[k].assign((size_t)nf + 1, 0);
        for (int64_t a = 0; a < nf; ++a) {
            const int k = cls_of(from_idx[a]);
            for (int q = 0; q < 3; ++q) pre[q][(size_t)a + 1] = pre[q][(size_t)a] + (q == k ? 1 : 0);
            const uint32_t m = c->rows.h_slot_meta[(size_t)from_idx[a]];
            const int n = (int)(m & 7);
            if ((n == 1 || n == 2) && (((m >> 3) & ((2u << n) - 1u)) != ((2u << n) - 1u))) hb.lo.band_full = 1;
            if (n == 0) hb.lo.band_full = 1;   // SNPs without a row sit among the one-row SNPs in the row list but last in the tiles
            if (n == 0) no_rowless = false;
        }
        for (int64_t b2 = 0; b2 < nt; ++b2) {
            const uint32_t m = c->rows.h_slot_meta[(size_t)to_idx[b2]];
            const int n = (int)(m & 7);
            if (n == 0) no_rowless = false;
            if ((n == 1 || n == 2) && (((m >> 3) & ((2u << n) - 1u)) != ((2u << n) - 1u))) hb.lo.band_full = 1;
        }
        {   // first row of each class region of the from-side row list (build_side: classes 1, 2, 4 in this order, 32-row aligned)
            int64_t rows = 0;
            for (int k = 0; k < 3; ++k) {
                base[k] = (int32_t)rows;
                rows += (int64_t)pre[k][(size_t)nf] * (1 << k);
                rows = (rows + 31) / 32 * 32;
            }
        }
        auto mark = [&](int64_t t0, int64_t t1, int64_t f0, int64_t f1) {
            for (int64_t ty = t0 / TILE; ty <= (t1 - 1) / TILE; ++ty)
                for (int64_t tx = f0 / 64; tx <= (f1 - 1) / 64; ++tx) band[(size_t)ty * ntx + tx] = 1;
        };
        std::vector<int32_t> nxt1, prv1;   // first one-row SNP at or after / last one before a list position (ordered rows only)
        if (hb.n_sr_blk > 0 && !hb.lo.band_full && ord_f) {
            nxt1.assign((size_t)nf + 1, (int32_t)nf);
            prv1.assign((size_t)nf + 1, -1);
            for (int64_t a = nf - 1; a >= 0; --a) nxt1[(size_t)a] = cls_of(from_idx[a]) == 0 ? (int32_t)a : nxt1[(size_t)a + 1];
            for (int64_t a = 0; a < nf; ++a) prv1[(size_t)a + 1] = cls_of(from_idx[a]) == 0 ? (int32_t)a : prv1[(size_t)a];
        }
        if (hb.n_sr_blk > 0 && !hb.lo.band_full)
            for (int64_t b2 = 0; b2 < nt; ++b2) {
                const ColInfo &ci = cols[(size_t)b2];
                const int64_t rb0 = ST.lrow[(size_t)b2], rb1 = rb0 + (1 << cls_of(to_idx[b2]));
                for (int iv = 0; iv < 3; ++iv) {
                    if (ci.e[iv] <= ci.s[iv]) continue;
                    for (int k = 0; k < 3; ++k) {
                        const int32_t n0 = pre[k][(size_t)ci.s[iv]], n1 = pre[k][(size_t)ci.e[iv]];
                        if (n1 <= n0) continue;
                        // a listed unit is evaluated whole: all 64 from-side SNPs of its epilogue tile (build_perm_tiles: 64 SNPs of
                        // one class in list order = 64 << k consecutive rows), so the range grows to whole tiles; the tiles of the
                        // SNPs with 3 and 4 rows are ordered differently from their rows: their whole class region is kept
                        int64_t f0 = base[k] + (int64_t)(n0 / 64 * 64) * (1 << k), f1 = base[k] + (int64_t)((n1 + 63) / 64 * 64) * (1 << k);
                        if (k == 0 && ord_f) {
                            // ordered rows: the partners (corner SNPs, in list order among themselves) start at the row of the first
                            // one-row SNP of the interval and end at that of the last
                            const int64_t first = nxt1[(size_t)ci.s[iv]], last = prv1[(size_t)ci.e[iv]];
                            f0 = (int64_t)SF.lrow[(size_t)first] / 64 * 64;
                            f1 = ((int64_t)SF.lrow[(size_t)last] + 1 + 63) / 64 * 64;
                        }
                        if (k == 2) {
                            f0 = base[2];
                            f1 = base[2] + (int64_t)pre[2][(size_t)nf] * 4;
                        }
                        if (f1 > hb.RFpad) f1 = hb.RFpad;
                        mark(rb0, rb1, f0, f1);
                        if (hb.diag) mark(f0, f1, rb0, rb1);   // a pair may be read in mirrored roles (g_entry)
                    }
                }
            }
    }
    hb.lo.fuse_ok = no_rowless ? 1 : 0;
    hb.lo.ordered = ord_f != nullptr ? 1 : 0;
}

// r06: the band's tiles as a LIST for the exact GEMM's launch (gemm_bits_kernel: a 1-D grid of the live tiles instead of the whole grid behind a mask);
// tiles above the diagonal of a diagonal block are left out as the kernel leaves them out; a band that covers most of the grid keeps the mask alone
bool PrepWork::band_list() {
    bool listed = false;
    const int64_t ntx = hb.RFpad / 64;
    if (hb.n_sr_blk > 0 && !hb.lo.band_full && hb.RTpad / TILE < 65536 && ntx < 65536) {
        const int64_t nty = hb.RTpad / TILE;
        for (int64_t ty = 0; ty < nty; ++ty)
            for (int64_t tx = 0; tx < ntx; ++tx)
                if (band[(size_t)ty * ntx + tx] && !(hb.diag && tx * 64 + 63 < ty * TILE)) bandl.push_back((uint32_t)(ty << 16 | tx));
        listed = bandl.size() * 2 <= band.size();
        if (!listed) bandl.clear();
    }
    hb.D.n_band = (int)bandl.size();
    return listed;
}

int prep_block(ldw_ctx *c, const int32_t *from_idx, int64_t nf, const int32_t *to_idx, int64_t nt, const ldw_mi_params *p,
               int slot, int64_t blk_no, HostBlock &hb, const SpanPlan *sp = nullptr, int pin_slot = -1, size_t stage_base = 0) {
    LDW_REQUIRE(nf > 0 && nt > 0, LDW_ERR_ARG, "empty block (nf=%lld nt=%lld)", (long long)nf, (long long)nt);
    LDW_REQUIRE(nf <= 1000000 && nt <= 1000000 && nf * nt < 2147483647LL, LDW_ERR_ARG, "block too large (%lld x %lld)",
                (long long)nf, (long long)nt);
    for (int64_t k = 0; k < nf; ++k)
        LDW_REQUIRE(from_idx[k] >= 0 && from_idx[k] < c->L, LDW_ERR_ARG, "SNP index %d out of range", from_idx[k]);
    for (int64_t k = 0; k < nt; ++k)
        LDW_REQUIRE(to_idx[k] >= 0 && to_idx[k] < c->L, LDW_ERR_ARG, "SNP index %d out of range", to_idx[k]);
    const bool prep_timing = ldw::host_timing();
    auto pnow = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tp[8] = {pnow(), 0, 0, 0, 0, 0, 0, 0};
    hb = HostBlock();
    hb.nf = nf;
    hb.nt = nt;
    hb.slot = slot;
    hb.blk_no = blk_no;
    hb.pin_slot = pin_slot;
    hb.stage_base = stage_base;
    hb.diag = same_list(from_idx, nf, to_idx, nt);
    PrepWork W{c, from_idx, to_idx, nf, nt, hb};
    if (int rc = W.intervals(p, sp)) return rc;
    tp[1] = pnow();
    if (int rc = W.row_order(sp)) return rc;
    tp[2] = pnow();
    if (int rc = build_side(c, from_idx, nf, W.SF, W.ord_f)) return rc;
    if (int rc = build_side(c, to_idx, nt, W.ST, W.ord_t)) return rc;
    tp[3] = pnow();
    hb.RFpad = W.SF.Rpad;
    hb.RTpad = W.ST.Rpad;
    W.tiles(slot);
    if (int rc = W.join_cols()) return rc;   // (a diagonal block's intervals: n_lr_total and the band are their first readers)
    hb.n_lr_total = (hb.diag ? nf * (nf - 1) / 2 : nf * nt - std::min(nf, nt)) - hb.n_sr_blk;
    tp[4] = pnow();
    W.band_mask();
    tp[5] = pnow();
    const bool band_listed = W.band_list();
    StageImage &im = hb.img;
    im.array<&DevPtrs::idx_f>(from_idx, (size_t)nf);
    im.array<&DevPtrs::idx_t>(to_idx, (size_t)nt);
    im.array<&DevPtrs::rl_f>(W.SF.rowlist.data(), W.SF.rowlist.size());
    im.array<&DevPtrs::rl_t>(W.ST.rowlist.data(), W.ST.rowlist.size());
    im.array<&DevPtrs::lrow_f>(W.SF.lrow.data(), (size_t)nf);
    im.array<&DevPtrs::lrow_t>(W.ST.lrow.data(), (size_t)nt);
    im.array<&DevPtrs::perm>(W.pf.data(), W.pf.size());
    const size_t at_perm_t = im.array<&DevPtrs::perm_t>(nullptr, (size_t)nt);   // (build_perm writes it straight into the pinned buffer)
    im.array<&DevPtrs::cols>(W.cols.data(), W.cols.size());
    im.array<&DevPtrs::pos_f>(W.SF.pos.data(), W.SF.pos.size());
    im.array<&DevPtrs::pos_t>(W.ST.pos.data(), W.ST.pos.size());
    im.array<&DevPtrs::cls_f>(W.SF.cls.data(), W.SF.cls.size());
    im.array<&DevPtrs::cls_t>(W.ST.cls.data(), W.ST.cls.size());
    im.array<&DevPtrs::cmax_f>(W.cmax.data(), W.cmax.size());
    im.array<&DevPtrs::tile_base>(W.tbase.data(), W.tbase.size());
    im.array<&DevPtrs::tf_list>(W.tf.data(), W.tf.size());
    im.array<&DevPtrs::band_mask>(W.band.data(), W.band.size());
    if (band_listed) im.array<&DevPtrs::band_list>(W.bandl.data(), W.bandl.size());
    hb.total = im.bytes;
    const int ps = pin_slot >= 0 ? pin_slot : slot;
    if (c->pin[ps].cap < stage_base + hb.total)   // (kept: the images in front of it, the first cold-start probe's)
        if (int rc = c->pin[ps].reserve_keep((stage_base + hb.total) * 2, stage_base)) return rc;
    tp[6] = pnow();
    char *b = c->pin[ps].as<char>() + stage_base;
    im.copy_to(b);
    build_perm(c, to_idx, nt, reinterpret_cast<int32_t *>(b + at_perm_t), W.ord_t);
    if (prep_timing && blk_no < 12)
        fprintf(stderr, "[ldw prep us] block %lld%s %lld x %lld span %d: checks + intervals %.0f  row order %.0f  sides %.0f  tiles + classes %.0f  band %.0f  band list %.0f  copy to staging %.0f  (%zu bytes)\n",
                (long long)blk_no, hb.diag ? " diag" : "", (long long)nf, (long long)nt, hb.span, tp[1] - tp[0], tp[2] - tp[1], tp[3] - tp[2], tp[4] - tp[3], tp[5] - tp[4], tp[6] - tp[5], pnow() - tp[6], hb.total);
    return LDW_OK;
}

int launch_gather(ldw_ctx *c, const HostBlock &hb, const EmitArgs &E, const SmallLayout &sl) {
    GatherArgs S;
    S.MI = c->MIblk.as<double>();
    S.cols = E.cols;
    S.nf = (int)hb.nf;
    S.nt = (int)hb.nt;
    S.lower_only = E.lower_only;
    hipLaunchKernelGGL(k_lr_gather, dim3((unsigned)((hb.nt + 15) / 16)), dim3(256), 0, c->stream, S, sl.pick[hb.slot], E.ckey, E.cval);
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

// Bound of |MI(exact sums) - MI(high-limb sums)| in nats.  Every cell of a joint table — indicator-row cell or derived by
// subtraction from the high-limb marginals — misses exactly the low limbs of ITS sequences, so sum_cells |dp| <= lo_abs_sum;
// dMI <= (1/den) sum_cells |dp| (|ln(pxy den / d)| + 1) with 0.5 <= pxy <= den, 0.25 <= d <= den^2, den >= neff.
double lo_bound(const ldw_ctx *c) {
    const double den = c->wts.neff > 1.0 ? c->wts.neff : 1.0;
    return c->wts.lo_abs_sum * (2.0 * std::log(den + 12.5) + 3.0) / den;
}

// what the emission of a block's pairs needs (short-range table, candidate list of this slot)
int make_emit_args(ldw_ctx *c, HostBlock &hb, const ldw_mi_params *p, const SmallLayout &sl, int spec_B) {
    const int s = hb.slot;
    const bool do_lr = !p->sr_only;
    EmitArgs E;
    memset(&E, 0, sizeof(E));
    E.cols = hb.D.cols;
    E.nf = (int)hb.nf;
    E.lower_only = hb.diag ? 1 : 0;
    E.keep_sr = p->keep_sr ? 1 : 0;
    E.do_lr = do_lr ? 1 : 0;
    E.sr_base = c->early_sr ? hb.sr_base : c->links.n_sr;   // (early_sr: the rows were assigned when the item was submitted)
    E.sr_a = c->links.sr_a.as<int32_t>();
    E.sr_b = c->links.sr_b.as<int32_t>();
    E.sr_mi = c->links.sr_mi.as<double>();
    // Long-range candidates: with a bucket guess from an earlier block the epilogue appends them itself and the
    // dense MI block is neither written nor re-read; without one (first block, histogram engine) the dense block
    // is written and k_lr_gather collects them once the true bucket is known.
    hb.spec_B = spec_B;
    size_t cap = (size_t)hb.nf * hb.nt;  // worst case: every pair of the block
    if (hb.span) {
        // a span only ever runs speculatively: a segment's candidates all come from the span's pair lists (a segment whose guess was
        // wrong is redone on its own, with its own worst-case list)
        size_t seg_max = 0;
        for (int k = 0; k < hb.span; ++k) seg_max = std::max(seg_max, (size_t)hb.nf * (size_t)hb.seg_nt[k]);
        hb.cand_cap = std::min<size_t>(seg_max, (size_t)PAIR_PATHS * PAIR_SHARDS * pair_cap_for(hb.nf, hb.nt, hb.span));
        cap = hb.cand_cap * (size_t)hb.span;
    }
    if (do_lr && !hb.force_plain) {
        if (int rc = c->cand_key[s].reserve(cap * 8)) return rc;
        if (int rc = c->cand_val[s].reserve(cap * 8)) return rc;
    }
    if (hb.span) {
        if (int rc = c->hist[s].reserve((size_t)hb.span * NBINS * 8)) return rc;
        for (int k = 0; k < hb.span; ++k) {
            ldw::PickOut *pk = reinterpret_cast<ldw::PickOut *>(reinterpret_cast<char *>(sl.pick[s]) + (size_t)k * PICK_STRIDE);
            hb.sseg[k].n_cand = &pk->n_cand;
            hb.sseg[k].ckey = c->cand_key[s].as<uint64_t>() + (size_t)k * hb.cand_cap;
            hb.sseg[k].cval = c->cand_val[s].as<uint64_t>() + (size_t)k * hb.cand_cap;
            hb.sseg[k].ghist = c->hist[s].as<unsigned long long>() + (size_t)k * NBINS;
        }
    }
    E.write_dense = (do_lr && hb.spec_B < 0) ? 1 : 0;   // the dense block only feeds k_lr_gather; SR-only passes take the screen path
    E.spec_B = hb.spec_B;
    E.spec_lo = hb.spec_B > 0 ? bucket_lo(hb.spec_B) : -1e300;
    E.any_sr = hb.n_sr_blk > 0 ? 1 : 0;
    E.n_cand = &sl.pick[s]->n_cand;
    E.ckey = c->cand_key[s].as<uint64_t>();
    E.cval = c->cand_val[s].as<uint64_t>();
    if (hb.force_plain && do_lr) {
        // a span's segment redone on its own: the slot's candidate buffers still hold the lists of the span's later segments
        if (int rc = c->miss_key.reserve((size_t)hb.nf * hb.nt * 8)) return rc;
        if (int rc = c->miss_val.reserve((size_t)hb.nf * hb.nt * 8)) return rc;
        E.ckey = c->miss_key.as<uint64_t>();
        E.cval = c->miss_val.as<uint64_t>();
    }
    // fp32 screen: only where a pair can be dismissed at all (speculative mode with a positive lower edge)
    E.scr_mode = (hb.spec_B > 0 || !do_lr) && !E.write_dense && (!do_lr || speculation_pays(c, p)) ? c->knobs.screen : 0;   // (no screen where nearly every unit would be listed)
    // the screen reads the top 31 bits of a joint sum; in the mixed-precision path the sums are those of the high-limb
    // weights (units of 2^(16 - F)) and the margin also covers what the low limbs can add (lo_bound)
    const int64_t tot = hb.mixed ? c->wts.total_fixed_hi : c->wts.total_fixed;
    int bits = 0;
    while (bits < 62 && (tot >> bits) != 0) ++bits;
    E.scr_shift = bits > 31 ? bits - 31 : 0;
    E.scr_scale = (float)std::ldexp(1.0, E.scr_shift - c->wts.frac_bits + (hb.mixed ? 8 * LO_LIMBS : 0));
    E.scr_eps = SCREEN_EPS + (hb.mixed ? (float)lo_bound(c) : 0.0f);
    if (hb.apx) {
        apx_screen_params(c, E);   // (ldw_epi.h: shared with the test hook ldw_debug_apx_params, so that the brute-force tests price the engine's own constants)
    }
    E.scr_viol = reinterpret_cast<unsigned long long *>(sl.lr_count + 1);
    hb.E = E;
    return LDW_OK;
}

// bucket pick + copy-back of the pick of slot s on `st`
int launch_pick(ldw_ctx *c, const HostBlock &hb, const ldw_mi_params *p, const SmallLayout &sl, hipStream_t st) {
    const int s = hb.slot;
    const unsigned int *pl_hdr = c->pairs[s].as<unsigned int>();   // (PairsLayout::hdr opens the buffer)
    if (hb.span) {
        PickSpanArgs S;
        memset(&S, 0, sizeof(S));
        for (int k = 0; k < hb.span; ++k) S.n_total[k] = (long long)hb.seg_lr_total[k];
        hipLaunchKernelGGL(k_pick_bucket_span, dim3((unsigned)hb.span), dim3(256), 0, st, c->hist[s].as<unsigned long long>(), p->lr_retain_links,
                           p->lr_links_approx, hb.spec_B, S, reinterpret_cast<char *>(sl.pick[s]), PICK_STRIDE,
                           pl_hdr, pair_cap_for(hb.nf, hb.nt, hb.span));
        LDW_HIP(hipGetLastError());
        return LDW_OK;
    }
    if (!p->sr_only) {
        const bool pl = hb.apx && c->knobs.screen == 1;
        hipLaunchKernelGGL(k_pick_bucket, dim3(1), dim3(256), 0, st, c->hist[s].as<unsigned long long>(), p->lr_retain_links,
                           p->lr_links_approx, hb.spec_B, (long long)hb.n_lr_total, sl.pick[s],
                           pl ? pl_hdr : nullptr, pair_cap_for(hb.nf, hb.nt));
        LDW_HIP(hipGetLastError());
    }
    return LDW_OK;
}

// the device image of a block's index structures is its part of the item's staging buffer: after that buffer's reserve, which may move it
static void fill_dev_ptrs(ldw_ctx *c, HostBlock &hb) {
    hb.img.bind(hb.D, c->dstage[hb.pin_slot >= 0 ? hb.pin_slot : hb.slot].as<char>() + hb.stage_base);
}

// The upload alone (copy stream): it needs no bucket guess, so the first item of a cold pass sends its lists while the cold-start probe of its
// kind is still running (ldw_mi_all_pairs); every other item uploads as the first step of submit_a.
int submit_upload(ldw_ctx *c, HostBlock &hb) {
    if (hb.uploaded) return LDW_OK;
    const int s = hb.slot;
    const int stg = hb.pin_slot >= 0 ? hb.pin_slot : s;   // (a span's segment that runs on its own is staged through the extra buffer)
    if (int rc = c->dstage[stg].reserve(hb.total)) return rc;
    // the device image and the per-slot buffers (G, histogram, pick, candidates) were last used by the block two steps back
    if (c->done_recorded[s]) LDW_HIP(hipStreamWaitEvent(c->copy_stream, c->ev_done[s], 0));
    LDW_HIP(hipMemcpyAsync(c->dstage[stg].p, c->pin[stg], hb.total, hipMemcpyHostToDevice, c->copy_stream));
    LDW_HIP(hipEventRecord(c->ev_up[s], c->copy_stream));
    c->up_recorded[s] = true;
    fill_dev_ptrs(c, hb);
    hb.uploaded = true;
    return LDW_OK;
}

// First phase: upload the block's index structures, then the co-occurrence GEMM into this slot's G buffer on the GEMM stream.
// Nothing there touches what the previous block's epilogue / selection still uses, so it overlaps the tail of block b.
int submit_a(ldw_ctx *c, HostBlock &hb, const ldw_mi_params *p, const SmallLayout &sl) {
    const int s = hb.slot;
    if (int rc = submit_upload(c, hb)) return rc;
    hb.submitted = true;
    if (c->knobs.engine != LDW_ENGINE_MFMA || hb.generic) return LDW_OK;
    hipStream_t gs = c->knobs.overlap ? c->gemm_stream : c->stream;   // overlap off: the stages of all blocks run back to back
    LDW_HIP(hipStreamWaitEvent(gs, c->ev_up[s], 0));
    if (c->done_recorded[s]) LDW_HIP(hipStreamWaitEvent(gs, c->ev_done[s], 0));
    const hipEvent_t *ev = handles(&c->ev_pool[(size_t)hb.blk_no * EVB]);
    const bool do_lr = !p->sr_only;
    // (a span: one guess serves every reference block, and the next guess only arrives after all of them.  No wider margin is needed: at C5
    // (800 kept rows per block, the noisiest thresholds) 3 of 1275 blocks miss per pass, as many as block by block)
    const int guess = do_lr ? ((speculation_pays(c, p) && !hb.force_plain) ? c->spec.spec_B_next[hb.diag ? 1 : 0] : -1) : 0;
    if ((int64_t)c->ev_valid.size() < hb.blk_no + std::max(1, hb.span)) c->ev_valid.resize((size_t)(hb.blk_no + std::max(1, hb.span)), 1);
    c->ev_valid[(size_t)hb.blk_no] = 1;
    for (int k = 1; k < hb.span; ++k) c->ev_valid[(size_t)hb.blk_no + k] = 0;   // (the span's stage events are its first block's; a segment that runs alone records its own)
    if (c->early_sr) {   // this pass assigns short-range rows in SUBMIT order (= block order)
        const int64_t sr_add = p->keep_sr ? hb.n_sr_blk : 0;
        if (int rc = ensure_links_capacity(c, c->links.n_sr + sr_add, c->links.n_lr)) return rc;
        hb.sr_base = c->links.n_sr;
        c->links.n_sr += sr_add;
    }
    if (hb.span) {
        // a span runs the approximate path or not at all: should the state it was planned on have gone (no positive guess any more),
        // its reference blocks take the ordinary chain one after the other (finish_span)
        const bool can = c->knobs.path_mode != 1 && c->apx.apx_ok && c->knobs.screen == 1 && do_lr && guess > 0;
        if (!can) {
            hb.span_alone = true;
            return LDW_OK;
        }
    }
    c->cnt.blocks_run += hb.span ? hb.span : 1;
    hb.guess = guess;
    // mixed precision: with a bucket guess the block will run the screen, which only needs the high limbs; the low
    // limbs follow for the listed units only.  The guess is frozen here because the GEMM commits to it.
    hb.mixed = c->knobs.mixed && c->knobs.screen && c->wts.nlimbs == HI_LIMBS + LO_LIMBS && do_lr && guess > 0 && lo_bound(c) < 1e-3 &&
               c->N <= 60000;   // the low-limb sums are int32: |sum| <= N * 2^15
    // approximate GEMM + class-wise popcounts: any block that takes the screen path (a bucket guess exists, or the pass
    // is SR-only and needs no MI to screen at all)
    hb.apx = c->knobs.path_mode != 1 && c->apx.apx_ok && c->knobs.screen && (do_lr ? guess > 0 : true) && hb.nt < (1 << 29);
    LDW_REQUIRE(c->knobs.path_mode != 2 || hb.apx || (do_lr && guess <= 0), LDW_ERR_STATE,
                "ldw_set_path(2): the approximate path is not available (delta %.3g, %d weight classes, %lld sequences, screen %d)", c->apx.apx_delta,
                c->apx.n_classes, (long long)c->N, c->knobs.screen);
    if (hb.apx) {
        hb.mixed = false;
        hb.lo.apx = 1;
        c->cnt.apx_blocks += hb.span ? hb.span : 1;
    }
    if (hb.span) {
        ++c->cnt.span_items;
        c->cnt.span_blocks += hb.span;
    }
    if (hb.mixed) ++c->cnt.mixed_blocks;
    if (hb.apx) {
        // phase 1 of the approximate path: panels, GEMM, SNP constants and the screens, all beside the previous block's tail.
        // The emission constants of phase 2 (table pointers, row base) are refreshed in submit_b.
        if (int rc = make_emit_args(c, hb, p, sl, do_lr ? guess : -1)) return rc;
        if (int rc = c->hist[s].reserve((size_t)NBINS * 8 * (size_t)(hb.span ? hb.span : 1))) return rc;
        hb.lo.span = hb.span;
        hb.lo.sseg = hb.sseg;
        if (int rc = launch_block_apx(c, hb.D, hb.nf, hb.nt, hb.RFpad, hb.RTpad, p->quirk_mode, hb.E, ev, 1, gs, nullptr, &hb.lo, c->hist[s].p, sl.pick[s],
                                      PICK_STRIDE * (size_t)(hb.span ? hb.span : 1)))
            return rc;
        LDW_HIP(hipEventRecord(c->ev_gemm[s], gs));
        return LDW_OK;
    }
    EmitArgs E;
    memset(&E, 0, sizeof(E));
    E.lower_only = hb.diag ? 1 : 0;
    E.do_lr = do_lr ? 1 : 0;
    if (int rc = launch_block_mi(c, hb.D, hb.nf, hb.nt, hb.RFpad, hb.RTpad, p->quirk_mode, E, ev, 1, &gx(c, s), gs, nullptr,
                                 hb.mixed ? &hb.lo : nullptr))
        return rc;
    LDW_HIP(hipEventRecord(c->ev_gemm[s], gs));
    return LDW_OK;
}

// Second phase: epilogue, histogram pick and the copy-back of the pick on the main stream.
// A block in generic order (HostBlock::generic): dense MI of every pair by the plain path, then the reference's pair list from the
// dense block with the len predicate (k_gen_count -> host scan of the 2 nt column counts -> k_gen_emit_sr, k_pick_bucket,
// k_gen_gather).  Synchronous where it needs the counts; such blocks are the exception (the reference's own parser emits ascending
// positions), correctness is what matters here.
int submit_generic(ldw_ctx *c, HostBlock &hb, const ldw_mi_params *p, const SmallLayout &sl) {
    const int s = hb.slot;
    const bool do_lr = !p->sr_only;
    LDW_HIP(hipStreamWaitEvent(c->stream, c->ev_up[s], 0));
    const hipEvent_t *ev = handles(&c->ev_pool[(size_t)hb.blk_no * EVB]);
    EmitArgs E0;
    memset(&E0, 0, sizeof(E0));
    E0.write_dense = 1;
    E0.spec_B = -1;
    E0.lower_only = 0;   // every entry of the block (a diagonal block too: the pair list decides which ones are pairs)
    if (int rc = launch_block_mi(c, hb.D, hb.nf, hb.nt, hb.RFpad, hb.RTpad, p->quirk_mode, E0, ev, 3, &gx(c, s), nullptr, nullptr)) return rc;
    LDW_HIP(hipEventRecord(ev[5], c->stream));   // (ldw_links_end brackets ev[1] .. ev[5] and ev[4] .. ev[2]: every event of the block must be recorded)
    LDW_HIP(hipEventRecord(ev[4], c->stream));
    if (int rc = c->hist[s].reserve((size_t)NBINS * 8)) return rc;
    if (int rc = c->colcnt.reserve((size_t)hb.nt * 8 + (size_t)hb.nt * 16 + 64)) return rc;
    LDW_HIP(hipMemsetAsync(c->hist[s].p, 0, (size_t)NBINS * 8, c->stream));
    LDW_HIP(hipMemsetAsync(sl.pick[s], 0, sizeof(ldw::PickOut), c->stream));
    GenArgs S;
    S.MI = c->MIblk.as<double>();
    S.nf = (int)hb.nf;
    S.nt = (int)hb.nt;
    S.lower_only = hb.diag ? 1 : 0;
    S.keep_sr = p->keep_sr ? 1 : 0;
    S.do_lr = do_lr ? 1 : 0;
    S.idx_f = hb.D.idx_f;
    S.idx_t = hb.D.idx_t;
    S.POS = c->meta.POS.as<int32_t>();
    S.g = c->meta.g;
    S.sr_dist = p->sr_dist;
    int32_t *cnt_u = c->colcnt.as<int32_t>(), *cnt_l = cnt_u + hb.nt;
    int64_t *off_u = reinterpret_cast<int64_t *>(c->colcnt.as<char>() + (((size_t)hb.nt * 8 + 15) / 16 * 16)), *off_l = off_u + hb.nt;
    const unsigned gridc = (unsigned)((hb.nt + 3) / 4);
    hipLaunchKernelGGL(k_gen_count, dim3(gridc), dim3(256), 0, c->stream, S, cnt_u, cnt_l, c->hist[s].as<unsigned long long>());
    LDW_HIP(hipGetLastError());
    std::vector<int32_t> hc((size_t)hb.nt * 2);
    LDW_HIP(hipMemcpyAsync(hc.data(), cnt_u, (size_t)hb.nt * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    std::vector<int64_t> ho((size_t)hb.nt * 2);
    int64_t nu = 0, nl = 0;
    for (int64_t b = 0; b < hb.nt; ++b) nu += hc[(size_t)b];
    int64_t ru = 0, rl = nu;   // all upper rows first, then all lower rows
    for (int64_t b = 0; b < hb.nt; ++b) {
        ho[(size_t)b] = ru;
        ho[(size_t)hb.nt + b] = rl;
        ru += hc[(size_t)b];
        rl += hc[(size_t)hb.nt + b];
        nl += hc[(size_t)hb.nt + b];
    }
    hb.n_sr_blk = nu + nl;
    hb.n_lr_total = (hb.diag ? hb.nf * (hb.nf - 1) / 2 : hb.nf * hb.nt - std::min(hb.nf, hb.nt)) - hb.n_sr_blk;
    const int64_t sr_add = p->keep_sr ? hb.n_sr_blk : 0;
    if (int rc = ensure_links_capacity(c, c->links.n_sr + sr_add, c->links.n_lr)) return rc;
    if (sr_add > 0) {
        LDW_HIP(hipMemcpyAsync(off_u, ho.data(), (size_t)hb.nt * 16, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_gen_emit_sr, dim3(gridc), dim3(256), 0, c->stream, S, off_u, off_l, (int64_t)c->links.n_sr, c->links.sr_a.as<int32_t>(), c->links.sr_b.as<int32_t>(),
                           c->links.sr_mi.as<double>());
        LDW_HIP(hipGetLastError());
        LDW_HIP(hipStreamSynchronize(c->stream));   // (ho is a host vector: the copy must be done before it goes away)
    }
    c->links.n_sr += sr_add;
    hb.spec_B = -1;
    if (do_lr) {
        const size_t cap = (size_t)hb.nf * hb.nt;
        if (int rc = c->cand_key[s].reserve(cap * 8)) return rc;
        if (int rc = c->cand_val[s].reserve(cap * 8)) return rc;
        if (int rc = launch_pick(c, hb, p, sl, c->stream)) return rc;
        hipLaunchKernelGGL(k_gen_gather, dim3(gridc), dim3(256), 0, c->stream, S, sl.pick[s], c->cand_key[s].as<uint64_t>(), c->cand_val[s].as<uint64_t>());
        LDW_HIP(hipGetLastError());
    }
    LDW_HIP(hipEventRecord(ev[2], c->stream));
    LDW_HIP(hipMemcpyAsync(c->pin_pick[s], sl.pick[s], sizeof(ldw::PickOut), hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipEventRecord(c->ev_pick[s], c->stream));
    ++c->cnt.generic_blocks;
    return LDW_OK;
}

int submit_b(ldw_ctx *c, HostBlock &hb, const ldw_mi_params *p, const SmallLayout &sl) {
    if (hb.span_alone) return LDW_OK;
    if (hb.generic) return submit_generic(c, hb, p, sl);
    const int s = hb.slot;
    LDW_HIP(hipStreamWaitEvent(c->stream, c->ev_up[s], 0));
    if (c->knobs.engine == LDW_ENGINE_MFMA) LDW_HIP(hipStreamWaitEvent(c->stream, c->ev_gemm[s], 0));
    const bool do_lr = !p->sr_only;
    const int64_t sr_add = (p->keep_sr && !c->early_sr) ? hb.n_sr_blk : 0;   // (early_sr: assigned in submit_a)
    if (int rc = ensure_links_capacity(c, c->links.n_sr + sr_add, c->links.n_lr)) return rc;
    if (int rc = c->hist[s].reserve((size_t)NBINS * 8)) return rc;
    if (!hb.apx) LDW_HIP(hipMemsetAsync(c->hist[s].p, 0, (size_t)NBINS * 8, c->stream));   // (the approximate path zeroed both in its first phase: k_zero4)
    if (int rc = make_emit_args(c, hb, p, sl, (hb.mixed || hb.apx) ? (do_lr ? hb.guess : -1) : (do_lr ? c->spec.spec_B_next[hb.diag ? 1 : 0] : -1)))   // (the bit-plane histogram engine shares the epilogue: it speculates like the MFMA engine)
        return rc;
    if (!hb.apx) LDW_HIP(hipMemsetAsync(sl.pick[s], 0, sizeof(ldw::PickOut), c->stream));
    const hipEvent_t *ev = handles(&c->ev_pool[(size_t)hb.blk_no * EVB]);
    if (hb.apx) {
        hb.lo.span = hb.span;
        hb.lo.sseg = hb.sseg;
        if (int rc = launch_block_apx(c, hb.D, hb.nf, hb.nt, hb.RFpad, hb.RTpad, p->quirk_mode, hb.E, ev, 2, nullptr, c->hist[s].as<unsigned long long>(), &hb.lo))
            return rc;
    } else if (int rc = launch_block_mi(c, hb.D, hb.nf, hb.nt, hb.RFpad, hb.RTpad, p->quirk_mode, hb.E, ev, c->knobs.engine == LDW_ENGINE_MFMA ? 2 : 3,
                                        &gx(c, s), nullptr, c->hist[s].as<unsigned long long>(), hb.mixed ? &hb.lo : nullptr))
        return rc;
    c->links.n_sr += sr_add;
    if (int rc = launch_pick(c, hb, p, sl, c->stream)) return rc;
    if (do_lr && hb.spec_B < 0)
        if (int rc = launch_gather(c, hb, hb.E, sl)) return rc;
    LDW_HIP(hipMemcpyAsync(c->pin_pick[s], sl.pick[s], hb.span ? PICK_STRIDE * (size_t)hb.span : sizeof(ldw::PickOut), hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipEventRecord(c->ev_pick[s], c->stream));
    return LDW_OK;
}

// guesses for later blocks from the pick of a finished one: a little below this block's bucket
void update_guess(ldw_ctx *c, bool diag, const ldw::PickOut *hp, bool missed) {
    // buckets are 0.5 % wide: guess ~5 % below the threshold of the last block of the same kind.  Diagonal blocks
    // lose their closest pairs to the short-range table and sit ~8 % (16 buckets) lower than off-diagonal ones:
    // until a block of the other kind has been seen, its guess is derived from this one with a wider margin.
    const int kind = diag ? 1 : 0, other = kind ^ 1;
    // the margin follows what the thresholds of this kind have actually done: the spread of the last six of them plus two
    // buckets, between 4 and 10 (every bucket below the true one costs ~3000 more candidates on the C4 shape; a miss costs a
    // full non-speculative pass of the block, after which the history starts over)
    int &hn = c->spec.spec_hist_n[kind];
    if (missed) hn = 0;
    c->spec.spec_hist[kind][hn % 6] = hp->B_true;
    ++hn;
    int margin = 10;
    if (hn >= 3) {
        int lo = hp->B_true, hi = hp->B_true;
        for (int k = 0; k < (hn < 6 ? hn : 6); ++k) {
            lo = c->spec.spec_hist[kind][k] < lo ? c->spec.spec_hist[kind][k] : lo;
            hi = c->spec.spec_hist[kind][k] > hi ? c->spec.spec_hist[kind][k] : hi;
        }
        // few kept rows per block (many blocks: C5 keeps ~800 per block) make the threshold itself noisier
        const bool small = hp->n * (1.0 - hp->prob) < 5000.0;
        c->spec.spec_small[kind] = small;
        margin = hi - lo + (small ? 4 : 2);
        const int mmin = small ? 6 : 4;
        margin = margin < mmin ? mmin : (margin > 10 ? 10 : margin);
    }
    c->spec.spec_B_next[kind] = hp->B_true - margin > 0 ? hp->B_true - margin : 0;
    c->spec.spec_seen[kind] = true;
    if (!c->spec.spec_seen[other] && !c->spec.spec_probed[other]) {   // (a probed guess of the other kind is better than one derived from this kind)
        const int g = diag ? hp->B_true - 10 : hp->B_true - 16 - 2 * 10;
        c->spec.spec_B_next[other] = g > 0 ? g : 0;
    }
}

// The long-range selection of ONE reference block from its candidate list (m candidates; the pick record on the device knows the
// ranks): threshold, kept rows in the reference's row order appended at *lr_count, then k_block_done (running count, block stats).
struct SelIn {
    int64_t m, nf, nt, blk_no, n_sr_blk;
    uint64_t *ck, *cv;
    ldw::PickOut *pick;                 // device
    const int32_t *idx_f, *idx_t;       // device: the block's own index lists
};
// the selection's input for block k of an item (an ordinary block: k = 0) with m candidates
SelIn sel_in(ldw_ctx *c, const HostBlock &hb, const SmallLayout &sl, int k, int64_t m) {
    const int s = hb.slot;
    const bool sp = hb.span > 0;   // (every segment of a span is long-range-only)
    SelIn S;
    S.m = m;
    S.nf = hb.nf;
    S.nt = sp ? hb.seg_nt[k] : hb.nt;
    S.blk_no = hb.blk_no + k;
    S.n_sr_blk = sp ? 0 : hb.n_sr_blk;
    S.ck = sp ? hb.sseg[k].ckey : (hb.E.ckey ? hb.E.ckey : c->cand_key[s].as<uint64_t>());
    S.cv = sp ? hb.sseg[k].cval : (hb.E.cval ? hb.E.cval : c->cand_val[s].as<uint64_t>());
    S.pick = reinterpret_cast<ldw::PickOut *>(reinterpret_cast<char *>(sl.pick[s]) + (size_t)k * PICK_STRIDE);
    S.idx_f = hb.D.idx_f;
    S.idx_t = hb.D.idx_t + (sp ? hb.seg_start[k] : 0);
    return S;
}

// The three arrays of the sort-free selection (k_sel_thresh) stay all-zero between uses (k_sel_clear): first use, or a larger block or span
// than any before, reserves them and zeroes them afresh
int reserve_sel_scratch(ldw_ctx *c, size_t bitmap_bytes, size_t chunk_bytes, size_t prefix_bytes) {
    if (bitmap_bytes <= c->sel_bitmap.cap && chunk_bytes <= c->sel_chunks.cap && prefix_bytes <= c->sel_prefix.cap) return LDW_OK;
    if (int rc = c->sel_bitmap.reserve(bitmap_bytes)) return rc;
    if (int rc = c->sel_chunks.reserve(chunk_bytes)) return rc;
    if (int rc = c->sel_prefix.reserve(prefix_bytes)) return rc;
    LDW_HIP(hipMemsetAsync(c->sel_bitmap.p, 0, c->sel_bitmap.cap, c->stream));
    LDW_HIP(hipMemsetAsync(c->sel_chunks.p, 0, c->sel_chunks.cap, c->stream));
    LDW_HIP(hipMemsetAsync(c->sel_prefix.p, 0, c->sel_prefix.cap, c->stream));
    return LDW_OK;
}

int select_rows(ldw_ctx *c, const SelIn &S, bool do_lr, const SmallLayout &sl) {
    const int64_t m = do_lr ? S.m : 0;
    uint64_t *ck = S.ck, *cv = S.cv;
    const uint64_t sel_space = (uint64_t)S.nf * (uint64_t)S.nt;
    static const bool sel_fast_on = getenv("LDW_NO_FAST_SELECT") == nullptr;
    const long long n_words = (long long)((2 * sel_space + 31) / 32) + 1, n_chunks = (long long)((2 * sel_space + SEL_CHUNK_BITS - 1) / SEL_CHUNK_BITS) + 1;
    const long long n_super_ll = (n_chunks + SEL_SUPER - 1) / SEL_SUPER;
    if (do_lr && m > 0 && sel_fast_on && c->knobs.select_mode == 0 && m <= SEL_MAX && n_super_ll <= SEL_MAX_SUPER) {
        // the common case: radix select + bitmap ranks, four small launches, no sort (k_sel_thresh)
        if (int rc = ensure_links_capacity(c, c->links.n_sr, c->links.n_lr + m)) return rc;
        const int n_super = (int)n_super_ll;
        if (int rc = reserve_sel_scratch(c, (size_t)n_words * 4, (size_t)n_chunks * 4, (size_t)SEL_MAX_SUPER * 4)) return rc;
        uint32_t *bm = c->sel_bitmap.as<uint32_t>(), *cc = c->sel_chunks.as<uint32_t>(), *sc = c->sel_prefix.as<uint32_t>();
        const unsigned gridm = (unsigned)((m + 255) / 256);
        hipLaunchKernelGGL(k_sel_thresh, dim3(1), dim3(1024), 0, c->stream, ck, S.pick);
        hipLaunchKernelGGL(k_sel_mark, dim3(gridm), dim3(256), 0, c->stream, ck, cv, S.pick, sel_space, bm, cc, sc);
        hipLaunchKernelGGL(k_sel_scatter, dim3(gridm), dim3(256), 0, c->stream, ck, cv, S.pick, sel_space, bm, cc, sc, n_super, S.idx_f, S.idx_t, (int)S.nf,
                           sl.lr_count, c->links.lr_a.as<int32_t>(), c->links.lr_b.as<int32_t>(), c->links.lr_mi.as<double>());
        hipLaunchKernelGGL(k_sel_clear, dim3(gridm), dim3(256), 0, c->stream, ck, cv, S.pick, sel_space, bm, cc, sc);
        LDW_HIP(hipGetLastError());
        c->links.n_lr += m;  // upper bound; the exact value is *lr_count
    } else if (do_lr && m > 0) {
        LDW_REQUIRE(m < 2147483647LL, LDW_ERR_SIZE, "too many quantile candidates (%lld)", (long long)m);
        if (int rc = ensure_links_capacity(c, c->links.n_sr, c->links.n_lr + m)) return rc;
        if (int rc = c->cand_key2.reserve((size_t)m * 8)) return rc;
        if (int rc = c->cand_val2.reserve((size_t)m * 8)) return rc;
        size_t tmp_bytes = 0;
        LDW_HIP(prim_sort_pairs(nullptr, tmp_bytes, ck, c->cand_key2.as<uint64_t>(), cv,
                                                   c->cand_val2.as<uint64_t>(), (int)m, 0, 64, c->stream));
        if (int rc = c->scratch.reserve(tmp_bytes)) return rc;
        LDW_HIP(prim_sort_pairs(c->scratch.p, tmp_bytes, ck, c->cand_key2.as<uint64_t>(), cv,
                                                   c->cand_val2.as<uint64_t>(), (int)m, 0, 64, c->stream));
        hipLaunchKernelGGL(k_lr_thresh, dim3(1), dim3(64), 0, c->stream, c->cand_key2.as<uint64_t>(), S.pick);
        LDW_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_lr_mark, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream,
                           c->cand_key2.as<uint64_t>(), c->cand_val2.as<uint64_t>(), S.pick, ck, cv, (long long)m);
        LDW_HIP(hipGetLastError());
        LDW_HIP(prim_sort_pairs(c->scratch.p, tmp_bytes, ck, c->cand_key2.as<uint64_t>(), cv,
                                                   c->cand_val2.as<uint64_t>(), (int)m, 0, 64, c->stream));
        hipLaunchKernelGGL(k_lr_append, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream,
                           c->cand_key2.as<uint64_t>(), c->cand_val2.as<uint64_t>(), S.pick, S.idx_f, S.idx_t, (int)S.nf,
                           sl.lr_count, c->links.lr_a.as<int32_t>(), c->links.lr_b.as<int32_t>(), c->links.lr_mi.as<double>());
        LDW_HIP(hipGetLastError());
        c->links.n_lr += m;  // upper bound; the exact value is *lr_count
    } else if (do_lr) {
        hipLaunchKernelGGL(k_lr_thresh, dim3(1), dim3(64), 0, c->stream, ck, S.pick);
        LDW_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_block_done, dim3(1), dim3(64), 0, c->stream, S.pick, sl.lr_count, S.n_sr_blk,
                       sl.stats_i + S.blk_no * 3, sl.stats_d + S.blk_no);
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

// the exact number of long-range rows kept by everything selected before (the copy-back the last queue_lr_count left)
int read_lr_count(ldw_ctx *c) {
    if (!c->lrc_recorded) return LDW_OK;
    LDW_HIP(hipEventSynchronize(c->ev_lrc));
    memcpy(&c->links.n_lr, c->pin_lrc, 8);
    return LDW_OK;
}
int queue_lr_count(ldw_ctx *c, const SmallLayout &sl) {
    LDW_HIP(hipMemcpyAsync(c->pin_lrc, sl.lr_count, 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipEventRecord(c->ev_lrc, c->stream));
    c->lrc_recorded = true;
    return LDW_OK;
}
// the end of an item on the main stream: the row count goes back, its last stage event, its slot is free
int end_item(ldw_ctx *c, const HostBlock &hb, const SmallLayout &sl) {
    if (int rc = queue_lr_count(c, sl)) return rc;
    LDW_HIP(hipEventRecord(c->ev_pool[(size_t)hb.blk_no * EVB + 3], c->stream));
    LDW_HIP(hipEventRecord(c->ev_done[hb.slot], c->stream));
    c->done_recorded[hb.slot] = true;
    return LDW_OK;
}
// what block k of an item taught the host: the guess for later blocks of its kind, and its trace record
void note_block(ldw_ctx *c, const HostBlock &hb, int k, const ldw::PickOut *hp, bool do_lr, bool missed) {
    if (do_lr && hp->n > 0) update_guess(c, hb.diag, hp, missed);
    if ((int64_t)c->trace.size() <= hb.blk_no + k) c->trace.resize((size_t)(hb.blk_no + k) + 1);
    ldw::BlockTrace &tr = c->trace[(size_t)(hb.blk_no + k)];
    tr = ldw::BlockTrace();
    tr.diag = hb.diag ? 1 : 0;
    tr.guess = hb.guess;
    tr.B_true = do_lr ? hp->B_true : -1;
    tr.path = hb.span ? 4 : (hb.apx ? 2 : (hb.mixed ? 1 : 0));
    tr.missed = missed ? 1 : 0;
    tr.n_cand = do_lr ? (long long)hp->n_cand : 0;
}

int finish_span(ldw_ctx *c, HostBlock &hb, const ldw_mi_params *p, const SmallLayout &sl);

int finish_block(ldw_ctx *c, HostBlock &hb, const ldw_mi_params *p, const SmallLayout &sl) {
    if (hb.span) return finish_span(c, hb, p, sl);
    const bool do_lr = !p->sr_only;
    const int s = hb.slot;
    // ---- the one host round trip of the block: the candidate count sizes the sorts ----
    LDW_HIP(hipEventSynchronize(c->ev_pick[s]));
    ldw::PickOut *hp = c->pin_pick[s].as<ldw::PickOut>();
    bool missed = false;
    if (do_lr && hb.spec_B >= 0 && hp->n > 0 && !hp->spec_ok) {
        // the bucket guess was above the true bucket: redo the epilogue non-speculatively (the short-range rows are
        // already final): full histogram, dense store, then pick and gather with the true bucket.  The plain two-kernel
        // path still has G; the mixed-precision and the approximate ones have to run the (full) GEMM again.
        EmitArgs E = hb.E;
        E.write_dense = 1;
        E.spec_B = -1;
        E.keep_sr = 0;
        E.scr_mode = 0;   // every pair goes into the histogram
        hb.spec_B = -1;
        LDW_HIP(hipMemsetAsync(c->hist[s].p, 0, (size_t)NBINS * 8, c->stream));
        LDW_HIP(hipMemsetAsync(sl.pick[s], 0, sizeof(ldw::PickOut), c->stream));
        hipEvent_t dummy[6] = {c->ev[3], c->ev[3], c->ev[4], c->ev[3], c->ev[5], c->ev[3]};   // keep the block's stage events as they are
        E.apx = 0;
        if (int rc = launch_block_mi(c, hb.D, hb.nf, hb.nt, hb.RFpad, hb.RTpad, p->quirk_mode, E, dummy, (hb.mixed || hb.apx) ? 3 : 2,
                                     &gx(c, s), nullptr, c->hist[s].as<unsigned long long>()))
            return rc;
        if (int rc = launch_pick(c, hb, p, sl, c->stream)) return rc;
        if (int rc = launch_gather(c, hb, E, sl)) return rc;
        LDW_HIP(hipMemcpyAsync(c->pin_pick[s], sl.pick[s], sizeof(ldw::PickOut), hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
        ++c->cnt.spec_misses;
        note_overflow(c, hp->over);
        missed = true;
    }
    note_block(c, hb, 0, hp, do_lr, missed || hb.force_plain);   // (force_plain: the redo of a span's segment whose guess was wrong)
    if (int rc = read_lr_count(c)) return rc;   // (all EARLIER blocks)
    if (int rc = select_rows(c, sel_in(c, hb, sl, 0, do_lr ? (int64_t)hp->n_cand : 0), do_lr, sl)) return rc;
    return end_item(c, hb, sl);
}

// One reference block of a span through the ordinary per-block chain (prep -> submit_a -> submit_b -> finish_block), synchronously, on the
// device buffers of the span's slot but staged through the extra staging buffer: the span's own lists are still read by the selection of
// its other segments.  force_plain: non-speculatively (the segment's guess was wrong).
int run_block_alone(ldw_ctx *c, const HostBlock &span, int k, const ldw_mi_params *p, const SmallLayout &sl, bool force_plain) {
    HostBlock hb;
    const int32_t *ti = span.span_to.data() + span.seg_start[k];
    LDW_HIP(hipStreamSynchronize(c->stream));                        // the extra staging buffer: free (an earlier segment may have used it)
    if (c->gemm_stream) LDW_HIP(hipStreamSynchronize(c->gemm_stream));
    if (int rc = prep_block(c, span.span_from.data(), span.nf, ti, span.seg_nt[k], p, span.slot, span.blk_no + k, hb, nullptr, LDW_NSLOT)) return rc;
    hb.force_plain = force_plain;
    if (int rc = submit_a(c, hb, p, sl)) return rc;
    if (int rc = submit_b(c, hb, p, sl)) return rc;
    if (int rc = finish_block(c, hb, p, sl)) return rc;
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

// The second half of a span: ONE host round trip for the pick records of all its reference blocks, then per block — in make_blocks
// order, which is the order the reference appends in (R/computePairwiseMI.R:103-116, :362) — the guess update, the selection of its
// candidates into the long-range table and its stats.  A block whose guess turned out too high (or all of them, when a pair list
// overflowed) is redone on its own, non-speculatively, in its place in that order.
int finish_span(ldw_ctx *c, HostBlock &hb, const ldw_mi_params *p, const SmallLayout &sl) {
    const int s = hb.slot;
    if (hb.span_alone) {
        for (int k = 0; k < hb.span; ++k)
            if (int rc = run_block_alone(c, hb, k, p, sl, false)) return rc;
        LDW_HIP(hipEventRecord(c->ev_done[s], c->stream));
        c->done_recorded[s] = true;
        return LDW_OK;
    }
    LDW_HIP(hipEventSynchronize(c->ev_pick[s]));
    ldw::PickOut picks[LDW_SPAN_MAX];
    for (int k = 0; k < hb.span; ++k) memcpy(&picks[k], c->pin_pick[s].as<char>() + (size_t)k * PICK_STRIDE, sizeof(ldw::PickOut));
    if (int rc = read_lr_count(c)) return rc;   // (all EARLIER blocks; within the span: upper bounds add up)
    {
        static const bool trace_on = getenv("LDW_BLOCK_TRACE") != nullptr;
        if (trace_on && picks[0].n > 0 && !picks[0].spec_ok) {   // a span that missed: its pair-list counters (an overflowing list fails every segment)
            unsigned int pl[PAIR_PATHS * PAIR_SHARDS];
            LDW_HIP(hipMemcpy(pl, c->pairs[s].as<unsigned int>() + PH_COUNT, sizeof(pl), hipMemcpyDeviceToHost));   // (PairsLayout::hdr opens the buffer)
            fprintf(stderr, "[ldw span at block %lld] guess %d, %d segments, pair-list capacity %u, counters by path:", (long long)hb.blk_no, hb.guess, hb.span, pair_cap_for(hb.nf, hb.nt, hb.span));
            for (int pth = 0; pth < PAIR_PATHS; ++pth) {
                unsigned long long tot = 0, mx = 0;
                for (int sh2 = 0; sh2 < PAIR_SHARDS; ++sh2) {
                    tot += pl[pth * PAIR_SHARDS + sh2];
                    mx = std::max<unsigned long long>(mx, pl[pth * PAIR_SHARDS + sh2]);
                }
                fprintf(stderr, "  [%d] total %llu max %llu", pth, tot, mx);
            }
            fprintf(stderr, "\n");
        }
    }
    // the common case — every guess held, every candidate set fits the sort-free selection — takes ONE launch per stage for all segments
    static const bool sel_fast_on = getenv("LDW_NO_FAST_SELECT") == nullptr;
    bool batched = sel_fast_on && c->knobs.select_mode == 0;
    long long m_max = 0, m_sum = 0;
    for (int k = 0; k < hb.span && batched; ++k) {
        const ldw::PickOut *hp = &picks[k];
        const uint64_t space = (uint64_t)hb.nf * (uint64_t)hb.seg_nt[k];
        const long long n_chunks = (long long)((2 * space + SEL_CHUNK_BITS - 1) / SEL_CHUNK_BITS) + 1, n_super = (n_chunks + SEL_SUPER - 1) / SEL_SUPER;
        batched = !(hp->n > 0 && !hp->spec_ok) && (long long)hp->n_cand <= SEL_MAX && n_super <= SEL_MAX_SUPER && (size_t)hp->n_cand <= hb.cand_cap;
        m_max = std::max<long long>(m_max, (long long)hp->n_cand);
        m_sum += (long long)hp->n_cand;
    }
    if (batched) {
        SelSpan S;
        memset(&S, 0, sizeof(S));
        SpanDoneArgs DA;
        memset(&DA, 0, sizeof(DA));
        S.n = hb.span;
        size_t w_off = 0, c_off = 0;
        size_t woff[LDW_SPAN_MAX], coff[LDW_SPAN_MAX];
        for (int k = 0; k < hb.span; ++k) {
            const uint64_t space = (uint64_t)hb.nf * (uint64_t)hb.seg_nt[k];
            const size_t n_words = (size_t)((2 * space + 31) / 32) + 1, n_chunks = (size_t)((2 * space + SEL_CHUNK_BITS - 1) / SEL_CHUNK_BITS) + 1;
            woff[k] = w_off;
            coff[k] = c_off;
            w_off += (n_words + 63) / 64 * 64;
            c_off += (n_chunks + 63) / 64 * 64;
            S.space[k] = space;
            S.n_super[k] = (int)((n_chunks + SEL_SUPER - 1) / SEL_SUPER);
        }
        if (int rc = reserve_sel_scratch(c, w_off * 4, c_off * 4, (size_t)LDW_SPAN_MAX * SEL_MAX_SUPER * 4)) return rc;
        if (int rc = ensure_links_capacity(c, c->links.n_sr, c->links.n_lr + m_sum)) return rc;
        for (int k = 0; k < hb.span; ++k) {
            const ldw::PickOut *hp = &picks[k];
            note_block(c, hb, k, hp, true, false);
            const SelIn B = sel_in(c, hb, sl, k, (int64_t)hp->n_cand);
            S.ck[k] = B.ck;
            S.cv[k] = B.cv;
            S.pick[k] = B.pick;
            S.idx_t[k] = B.idx_t;
            S.bitmap[k] = c->sel_bitmap.as<uint32_t>() + woff[k];
            S.chunks[k] = c->sel_chunks.as<uint32_t>() + coff[k];
            S.supers[k] = c->sel_prefix.as<uint32_t>() + (size_t)k * SEL_MAX_SUPER;
        }
        const unsigned gridm = (unsigned)std::max<long long>(1, (m_max + 255) / 256);
        hipLaunchKernelGGL(k_sel_thresh_span, dim3(1, (unsigned)hb.span), dim3(1024), 0, c->stream, S);
        hipLaunchKernelGGL(k_sel_mark_span, dim3(gridm, (unsigned)hb.span), dim3(256), 0, c->stream, S);
        hipLaunchKernelGGL(k_sel_scatter_span, dim3(gridm, (unsigned)hb.span), dim3(256), 0, c->stream, S, hb.D.idx_f, (int)hb.nf,
                           sl.lr_count, c->links.lr_a.as<int32_t>(), c->links.lr_b.as<int32_t>(), c->links.lr_mi.as<double>());
        hipLaunchKernelGGL(k_sel_clear_span, dim3(gridm, (unsigned)hb.span), dim3(256), 0, c->stream, S);
        hipLaunchKernelGGL(k_span_done, dim3(1), dim3(64), 0, c->stream, S, DA, sl.lr_count, sl.stats_i + hb.blk_no * 3, sl.stats_d + hb.blk_no);
        LDW_HIP(hipGetLastError());
        c->links.n_lr += m_sum;   // upper bound; the exact value is *lr_count
    }
    for (int k = 0; k < hb.span && !batched; ++k) {
        const ldw::PickOut *hp = &picks[k];
        const bool missed = hp->n > 0 && !hp->spec_ok;
        if (missed) {
            ++c->cnt.spec_misses;
            ++c->cnt.span_fallbacks;
            note_overflow(c, hp->over);
            // (the redo reads the exact row count of everything before it: the selections of the span's earlier segments are queued, not counted yet)
            if (int rc = queue_lr_count(c, sl)) return rc;
            if (int rc = run_block_alone(c, hb, k, p, sl, true)) return rc;
            continue;
        }
        note_block(c, hb, k, hp, true, false);
        LDW_REQUIRE((size_t)hp->n_cand <= hb.cand_cap, LDW_ERR_STATE, "span segment %d lists %llu candidates, capacity %zu", k, (unsigned long long)hp->n_cand, hb.cand_cap);
        if (int rc = select_rows(c, sel_in(c, hb, sl, k, (int64_t)hp->n_cand), true, sl)) return rc;
    }
    return end_item(c, hb, sl);
}

// Cold start: a bucket guess for a block kind from a LATTICE SAMPLE of one of its blocks.  Every PROBE_STRIDE-th SNP of both sides
// (about 2000 per side, spanning the whole block, so the sample has the block's own mix of distances) is run through the plain
// path — full-limb GEMM of the sample's rows, fp64 MI of every sampled pair, histogram of the long-range ones, bucket pick — and the
// bucket that holds the type-7 rank of the SAMPLE becomes the guess, minus a margin for the sampling noise (~400-800 pairs in the
// tail: +-0.3 bucket) and for the block-to-block drift.  ~0.2 ms, nothing is emitted, no table or counter of the pass is touched.
// Without it the first block of a pass (and of every rank of a multi-GPU pass) takes the non-speculative path — 5-limb GEMM of the
// whole block, fp64 MI of all 1e8 pairs, radix sorts: 3x the time of a speculative block — and the next one cannot overlap it.
// A guess that turns out too high costs what it always costs: the block is redone non-speculatively (spec_misses).
constexpr int64_t PROBE_SIDE = 2048;          // sampled SNPs per side
constexpr int64_t PROBE_MIN_PAIRS = 16000000; // smaller blocks are cheap enough without a guess
constexpr int PROBE_MARGIN = 6;

// r04: in two halves, so that the probes of both kinds are queued back to back (1.25 ms of a cold pass went into two prep / upload / run /
// wait round trips).  Probe `which` (0, 1) uses the G buffer, histogram and pick record of pipeline slot `which`, and its own part of the
// EXTRA staging pair (pin / dstage [LDW_NSLOT], otherwise used by a span's segment that is redone on its own, which first drains the
// streams): the three slots' staging buffers belong to the helper threads and to item 0's upload from the start of the pass.
// Each probe records its own event (ev_probe[which]); the caller waits for the probes of slot 0 and of the first item's kind before it
// submits that item and collects the other one behind it (ldw_mi_all_pairs).
struct Probe {
    HostBlock hb;
    int kind = 0, which = 0;
    bool queued = false;
};
int probe_enqueue(ldw_ctx *c, const int32_t *fi, int64_t nf, const int32_t *ti, int64_t nt, const ldw_mi_params *p, const SmallLayout &sl, int kind, int which,
                  size_t pin_base, Probe &P) {
    const int64_t stride = std::max<int64_t>(1, std::max(nf, nt) / PROBE_SIDE);
    std::vector<int32_t> sf, st;
    for (int64_t k = 0; k < nf; k += stride) sf.push_back(fi[k]);
    for (int64_t k = 0; k < nt; k += stride) st.push_back(ti[k]);
    ldw_mi_params q = *p;
    q.keep_sr = 0;
    HostBlock &hb = P.hb;
    P.kind = kind;
    P.which = which;
    P.queued = false;
    constexpr int PS = LDW_NSLOT;
    if (int rc = prep_block(c, sf.data(), (int64_t)sf.size(), st.data(), (int64_t)st.size(), &q, which, 0, hb, nullptr, PS, pin_base)) return rc;
    if (hb.n_lr_total < 100000) return LDW_OK;   // too few long-range pairs in the sample to say anything
    if (c->dstage[PS].cap < pin_base + hb.total) {
        // (the first sample reserves room for both; should the second still not fit, the first one's kernels leave the buffer before it goes)
        if (which > 0) LDW_HIP(hipStreamSynchronize(c->stream));
        if (int rc = c->dstage[PS].reserve(which == 0 ? 2 * hb.total + 65536 + 256 : pin_base + hb.total)) return rc;
    }
    LDW_HIP(hipMemcpyAsync(c->dstage[PS].as<char>() + pin_base, c->pin[PS].as<char>() + pin_base, hb.total, hipMemcpyHostToDevice, c->stream));
    fill_dev_ptrs(c, hb);
    if (int rc = c->hist[which].reserve((size_t)NBINS * 8)) return rc;
    if (int rc = make_emit_args(c, hb, &q, sl, -1)) return rc;
    hb.E.write_dense = 0;   // nothing reads the sample's MI values: only the histogram of the long-range ones
    LDW_HIP(hipMemsetAsync(c->hist[which].p, 0, (size_t)NBINS * 8, c->stream));
    LDW_HIP(hipMemsetAsync(sl.pick[which], 0, sizeof(ldw::PickOut), c->stream));
    // (in the CALLER's reading of RXY: under quirk Q1 the scrambled RXY — r of two other SNPs — lifts 3-state x 3-state pairs into the tail of an
    // off-diagonal block; a sample evaluated with the intended RXY sat 15 buckets = 7.5 % below the block's own threshold)
    if (int rc = launch_block_mi(c, hb.D, hb.nf, hb.nt, hb.RFpad, hb.RTpad, p->quirk_mode, hb.E, handles(c->ev), 3, &gx(c, which), nullptr, c->hist[which].as<unsigned long long>()))
        return rc;
    hipLaunchKernelGGL(k_pick_bucket, dim3(1), dim3(256), 0, c->stream, c->hist[which].as<unsigned long long>(), p->lr_retain_links, p->lr_links_approx, -1,
                       (long long)hb.n_lr_total, sl.pick[which], (const unsigned int *)nullptr, 0u);
    LDW_HIP(hipGetLastError());
    LDW_HIP(hipMemcpyAsync(c->pin_pick[which], sl.pick[which], sizeof(ldw::PickOut), hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemsetAsync(sl.pick[which], 0, sizeof(ldw::PickOut), c->stream));
    LDW_HIP(hipEventRecord(c->ev_probe[which], c->stream));
    P.queued = true;
    return LDW_OK;
}
// after hipEventSynchronize(c->ev_probe[P.which])
void probe_collect(ldw_ctx *c, const Probe &P) {
    if (!P.queued) return;
    const ldw::PickOut *hp = c->pin_pick[P.which].as<ldw::PickOut>();
    if (hp->n > 0 && hp->B_true < NBINS) {
        const int g = hp->B_true - PROBE_MARGIN;
        c->spec.spec_B_next[P.kind] = g > 0 ? g : 0;
        c->spec.spec_hist_n[P.kind] = 0;
        c->spec.spec_probed[P.kind] = true;
        ++c->cnt.probe_blocks;
        static const bool trace_on = getenv("LDW_BLOCK_TRACE") != nullptr;
        if (trace_on) fprintf(stderr, "[ldw probe] kind %d: sample %lld x %lld, %lld long-range pairs, bucket %d -> guess %d\n", P.kind, (long long)P.hb.nf, (long long)P.hb.nt,
                              (long long)P.hb.n_lr_total, hp->B_true, c->spec.spec_B_next[P.kind]);
    }
}

// whether the next block can be submitted before the current one is finished
bool can_submit_early(ldw_ctx *c, const HostBlock &hb, const ldw_mi_params *p) {
    if (!c->knobs.overlap) return false;
    if (!p->sr_only && !speculation_pays(c, p)) return true;   // (plain blocks need no guess)
    // no bucket guess for this kind of block yet (the first blocks of a cold pass): the block in flight is about to provide one —
    // submitted now, this block would take the non-speculative path (full 5-limb GEMM, fp64 for every pair: ~4 ms more)
    return !(c->knobs.engine == LDW_ENGINE_MFMA && !p->sr_only && c->knobs.screen && c->spec.spec_B_next[hb.diag ? 1 : 0] < 0);
}


// The per-slot device buffers of a block's launch chain (launch_block_mi / launch_block_apx, ldw_mi_block.inc): the records they hold and ONE
// description of each buffer — a function of the block geometry that names every array once, with its element type and count.  The byte count
// that reserve_slot_buffers and the launch sites reserve, the typed pointers the kernels receive and the ranges k_zero4 clears all come from it.
// Plain C++, no HIP: tests/host/slot_layout_check.cpp reads this header with g++ (tests/test_slot_layout_host.py).
#pragma once
#include "ldw_carve.h"

namespace ldw {

// ------------------------------------------------------------------------------------------------
// the records
// ------------------------------------------------------------------------------------------------
// Short-range partners of one to-side SNP: up to three disjoint, ascending index intervals [s,e) of the
// from-side list, plus the first row of its upper (a_loc < b_loc) and lower (a_loc > b_loc) segment in
// the short-range table (relative to the block's base row).
struct ColInfo {
    int32_t s[3], e[3];
    int32_t pad[2];
    int64_t off_u, off_l;
};

// everything the epilogue needs about one to-side SNP, staged in LDS once per workgroup so that the
// per-pair loop has no dependent global loads except its G entries
struct ColMeta {
    int32_t sb;
    uint32_t mb;
    int32_t rb0, bl;   // first row position in the to-side row list; local index of the SNP in the to-side list
    double rb;      // r of the to-side SNP
    double rq;      // Q1 on square blocks: r[idx_f[b_loc]]
    double pYd[5];
    int64_t pb[5];
    float pYf[5];
    int32_t pad2;
#ifdef LDW_COLMETA_PAD   // measurement only: how sensitive are the screens to the size of the staged column?
    char padx[LDW_COLMETA_PAD];
#endif
    ColInfo ci;
};

// per-lane constants of the from-side SNP
struct RowSide {
    int sa, na;
    uint32_t ma;
    int64_t ra0;
    double ra, rta;  // rta: Q1 on square blocks, r[idx_t[a_loc]]
    int64_t pa[5];
    double pXd[5];
    float pXf[5];
};

struct RowPack {
    RowSide R;
    int32_t a_loc;   // local index in the from-side list, -1: padding slot of the tile
    int32_t pad;
};

// r05: what k_screen_maybe needs of a biallelic SNP, in 32 bytes instead of the ~200-byte ColMeta / RowPack (its entries arrive from the GEMM's
// epilogue in region order, ~17 M per span on data without rare states, and the kernel was bound by the gathers of the two full records:
// 1.32 ms per span).  Built by k_build_packs from the _hi packs (marginals of the APPROXIMATE weights: < 2^31 units); 0 / -1 for other SNPs.
struct MiniCol {
    int32_t pb0;        // approximate minor marginal (units of 2^e_last)
    float pY0, pY1;     // weighted marginals of the two states (ColMeta::pYf)
    float rb, rq;       // r of the SNP; Q1 on square blocks / spans: r[idx_f[b_loc]]
    int32_t bl, seg0;   // local index in its reference block; first to-side index of its segment (a span's ColInfo::pad[1])
    int32_t sb;
};
struct MiniRow {
    int32_t pa0, pa1;
    float pX0, pX1;
    float ra, rta;
    int32_t a_loc, sa;
};

// a listed candidate pair: from-slot index (64 * tile + lane), column slot, first bit row | row count << 29 of both SNPs
struct PairEnt {
    uint32_t t, q, ra, rb;
};
constexpr int PAIR_PATHS = 5;    // (NA, NB) = (1,1) (2,1) (1,2) (2,2) straight-line code, 4 = predicated
constexpr int PAIR_SHARDS = 8;

// an entry of the maybe list (ApxGemmArgs::maybe, ldw_apx.h)
struct ApxMaybe {
    uint32_t trow, fcol;   // row-list positions = column slot / from slot of the epilogue orders (biallelic rows: position == slot)
    int32_t n;             // the approximate joint sum n'
};
#ifndef LDW_MAYBE_MAX
#define LDW_MAYBE_MAX 96
#endif
constexpr int APX_MAYBE_MAX = LDW_MAYBE_MAX;   // more failing entries than this in a region of 2048: storing the region is the cheaper path

constexpr int LDW_SPAN_MAX = 8;   // most reference blocks of a span (ldw_epi.h)

// The header of a slot's pair lists (PairsLayout::hdr, zeroed per block), by 32-bit word
enum PairHdr : int {
    PH_COUNT = 0,                               // [PAIR_PATHS * PAIR_SHARDS] entries appended to each list (a list that overflowed counts past its capacity)
    PH_MAYBE_OVER = PAIR_PATHS * PAIR_SHARDS,   // set by k_screen_maybe when the maybe list overflowed; k_pick_bucket reads it with the counts
    PH_MAYBE_N = 48,                            // entries the GEMM's epilogue handed to the maybe list (0 when the list is off)
    PH_WORDS = 64
};
static_assert(PH_MAYBE_OVER < PH_MAYBE_N && PH_MAYBE_N < PH_WORDS, "the header holds the list counts, the overflow word and the maybe counter");
constexpr int UNIT_HDR_WORDS = 16;   // UnitsLayout::counters: words 0, 1 = entries of the two flat lists; the per-(tile, class) counters start here

// ------------------------------------------------------------------------------------------------
// the geometry of a block and the layouts that follow from it
// ------------------------------------------------------------------------------------------------
struct SlotGeom {
    int64_t nf = 1, nt = 1;             // SNPs of the from side and of the to side (a span: the concatenated to side)
    int64_t RFpad = 128, RTpad = 128;   // rows of the two row lists (build_side: multiples of 128)
    int64_t nf_tiles = 1;               // from-tiles of 64 slots in the epilogue order (build_perm_tiles)
    int nseg = 0;                       // reference blocks on the to side (0: an ordinary block)
    bool mixed = false;                 // mixed-precision path: per-(tile, class) counters and per-tile lists behind the flat unit lists
    int64_t nf_slots() const { return nf_tiles * 64; }
    int64_t n_units() const { return nf_tiles * nt; }   // a unit = one from-tile x one to-side SNP
};

// apx_packs[s] / packs: the per-block SNP constants in epilogue order (k_build_packs)
struct PacksLayout : Carve {
    Slot<ColMeta> cp, cp_hi;      // [nt] epilogue order perm_t; _hi: with the marginals of the high-limb / approximate weights
    Slot<RowPack> rp, rp_hi;      // [64 * from-tiles] epilogue order perm_f (padded)
    Slot<float> rloc_f, rloc_t;   // [nf] / [nt] r of the SNPs by LOCAL index (quirk Q1 on ragged blocks)
    explicit PacksLayout(const SlotGeom &g)
        : cp(take<ColMeta>(g.nt)), cp_hi(take<ColMeta>(g.nt)), rp(take<RowPack>(g.nf_slots())), rp_hi(take<RowPack>(g.nf_slots())),
          rloc_f(take<float>(g.nf)), rloc_t(take<float>(g.nt)) {}
};

// apx_units[s] / scr_units: what the screens list for the fp64 kernels
struct UnitsLayout : Carve {
    Slot<unsigned int> counters;   // UNIT_HDR_WORDS (entries of the two flat lists), mixed: + [from-tiles][3] listed units per (tile, class); zeroed per block
    Slot<uint64_t> flat;           // [2][n_units]: the straight-line units, the others
    Slot<uint32_t> tl;             // mixed: [from-tiles][nt] per-tile lists of column slots (LoGeom::tl)
    int64_t list_stride;           // entries between the two flat lists
    explicit UnitsLayout(const SlotGeom &g)
        : counters(take<unsigned int>(UNIT_HDR_WORDS + (g.mixed ? 3 * g.nf_tiles : 0))), flat(take<uint64_t>(2 * g.n_units())),
          tl(take<uint32_t>(g.mixed ? g.n_units() : 0)), list_stride(g.n_units()) {}
    unsigned int *tile_cnt() const { return counters + UNIT_HDR_WORDS; }
    Range zeroed() const { return cover(counters); }
};

// pairs[s]: the pair lists of the approximate screen and, behind them, the maybe list of the GEMM's epilogue (ApxGemmArgs::maybe)
struct PairsLayout : Carve {
    Slot<unsigned int> hdr;   // PairHdr; zeroed per block.  Taken first: the buffer opens with it (launch_pick, finish_span)
    Slot<PairEnt> lists;      // [PAIR_PATHS * PAIR_SHARDS][pl_cap], list = path * PAIR_SHARDS + shard
    Slot<ApxMaybe> maybe;     // [maybe_cap]
    PairsLayout(uint32_t pl_cap, uint32_t maybe_cap)
        : hdr(take<unsigned int>(PH_WORDS)), lists(take<PairEnt>((int64_t)PAIR_PATHS * PAIR_SHARDS * pl_cap)), maybe(take<ApxMaybe>(maybe_cap)) {}
    Range zeroed() const { return cover(hdr); }
};

// apx_bins[s]: what the approximate GEMM's epilogue and its tile pruning read by ROW of the two row lists, and the screen's flags by epilogue slot
struct BinsLayout : Carve {
    Slot<uint8_t> bin_t, bin_f;       // [RTpad] / [RFpad] bin of the threshold table (255: not a biallelic r = 2 SNP's row); k_build_packs writes every row
    Slot<uint8_t> rflag_t, rflag_f;   // [RTpad] / [RFpad] pruning flags (PF_*) by row; zeroed per block: k_build_packs writes the rows of SNPs only, padding rows read 0
    Slot<unsigned int> n_live;        // count of the wave tiles the pruning leaves (k_apx_live_tiles); zeroed per block, with the row flags
    Slot<uint8_t> sflag_t, sflag_f;   // [nt] / [64 * from-tiles] the same flags by epilogue slot (the screen reads them, in phase 2 where the GEMMs are long)
    Slot<uint32_t> tile_list;         // [RTpad / 64][RFpad / 64] the live tiles, one word each, at their finest: 64 x 64 wave tiles
    explicit BinsLayout(const SlotGeom &g)
        : bin_t(take<uint8_t>(g.RTpad)), bin_f(take<uint8_t>(g.RFpad)), rflag_t(take<uint8_t>(g.RTpad)), rflag_f(take<uint8_t>(g.RFpad)),
          n_live(take<unsigned int>(1)), sflag_t(take<uint8_t>(g.nt)), sflag_f(take<uint8_t>(g.nf_slots())),
          tile_list(take<uint32_t>((g.RTpad / 64) * (g.RFpad / 64))) {}
    Range zeroed() const { return cover(rflag_t, rflag_f, n_live); }
};

// apx_mini[s]: the 32-byte extracts of the _hi packs that k_screen_maybe reads (both phases)
struct MiniLayout : Carve {
    Slot<MiniCol> col;   // [nt]
    Slot<MiniRow> row;   // [64 * from-tiles]
    explicit MiniLayout(const SlotGeom &g) : col(take<MiniCol>(g.nt)), row(take<MiniRow>(g.nf_slots())) {}
};

// Entries of ONE pair list of a block (PAIR_PATHS x PAIR_SHARDS lists): an eighth of the block's pairs (a shard's fair share of ALL of them), between
// 2^12 and PAIR_CAP.  Small blocks (tests, several engines on one GPU) then take megabytes instead of the fixed 1.4 GB; a list that overflows makes
// the block fall back like a wrong guess (k_pick_bucket: spec_ok = 0), so results never depend on it.  nseg > 4: the lists of a span of that many
// reference blocks (about 4e4 listed pairs per 10k x 10k block, most of them in ONE of the five paths: 3-state x 3-state SNP pairs) get twice the room.
constexpr uint64_t PAIR_CAP = 1u << 18;
inline uint32_t pair_cap_of(int64_t nf, int64_t nt, int nseg) {
    const uint64_t top = nseg > 4 ? 2 * PAIR_CAP : PAIR_CAP;
    uint64_t want = (uint64_t)nf * (uint64_t)nt / PAIR_SHARDS + 1, cap = 1u << 12;
    while (cap < want && cap < top) cap <<= 1;
    return (uint32_t)cap;
}
// Entries of the maybe list of an item.  r05: the WORST case — every region of 32 to-rows x 64 from-rows of the row rectangle hands over
// APX_MAYBE_MAX entries (0.56 B per entry of G', a seventh of G' itself) — so the list cannot overflow whatever the data look like.
inline uint32_t maybe_cap_of(int64_t RTpad, int64_t RFpad) {
    return (uint32_t)std::min<int64_t>(((RTpad + 31) / 32) * ((RFpad + 63) / 64) * (int64_t)APX_MAYBE_MAX + 64, (int64_t)1 << 30);
}

// What reserve_slot_buffers sizes the slot buffers for, ahead of a pass of blocks of `blk` SNPs in spans of up to nseg: 1.25 rows per SNP + padding
// (a C4 block has 1.16), the classes of the from-side epilogue order padded to whole tiles.
inline SlotGeom slot_geom_estimate(int64_t blk, int64_t nseg) {
    SlotGeom g;
    g.nf = blk;
    g.nt = blk * nseg;
    g.RFpad = (g.nf * 5 / 4 + 512 + 127) / 128 * 128;
    g.RTpad = (g.nt * 5 / 4 + 512 + 127) / 128 * 128;
    g.nf_tiles = blk / 64 + 6;
    g.nseg = (int)nseg;
    return g;
}

}  // namespace ldw

// The geometry of the gathered low-limb GEMM of the mixed-precision path (gemm_lo_units_kernel, ldw_gemm_bits.hip; LoGeom, ldw_epi.h), as ONE host
// function: which low-limb rows the listed units of a (from-tile, row-slot class) get, how wide a tile's rows are, where its block starts and in
// which order the launch walks the (tile, fs) sub-tiles.  prep_block (PrepWork::tiles, ldw_mi_items.inc) lays a block out with it, and the test hook
// ldw_debug_lo_units (ldw_debug.hip) lays out caller-made unit lists with the same arithmetic.
// Plain C++ on the host: tests/host/lo_geom_check.cpp reads this header with g++ (tests/test_lo_geom_host.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define LDW_LO_FN __host__ __device__ __forceinline__
#else
#define LDW_LO_FN inline
#endif

namespace ldw {

// row-slot class of a SNP with `nrows` indicator rows: 0, 1, 2 = 1, 2, 4 row slots
LDW_LO_FN int lo_class(int nrows) { return nrows <= 1 ? 0 : (nrows == 2 ? 1 : 2); }

constexpr int LO_CHUNK_ROWS = 128;   // low-limb rows of one workgroup of the gathered GEMM (= TILE): a class's rows are padded to whole chunks
constexpr int LO_TILE_SNPS = 64;     // from-side SNPs (epilogue lanes) of a from-tile

struct LoLayout {
    int32_t n_lc[3] = {0, 0, 0};         // to-side SNPs per row-slot class
    int32_t uoff[3] = {0, 0, 0};         // first entry of a class in a tile's unit list (tl[tile * nt + uoff[lc] + k])
    int32_t rowbase[3] = {0, 0, 0};      // first low-limb row of a class: unit k of class lc owns rows rowbase[lc] + (k << lc) .. + (1 << lc)
    int32_t RTlo = 0;                    // low-limb rows per tile (the classes' rows, each padded to 128)
    int32_t ntiles = 0, n_tf = 0;        // from-tiles; (tile, fs) pairs of the launch
    int32_t n_tiles_cf[3] = {0, 0, 0};   // from-tiles whose widest row-slot class is 1, 2, 4
    int64_t glo_total = 0;               // ints of the whole low-limb buffer
};

// rows_to(k): indicator rows of to-side SNP k (0 <= k < nt).  rows_from_slot(t): indicator rows of the from-side SNP in lane t % 64 of from-tile
// t / 64 (0 <= t < n_slots, a multiple of 64), -1 for a padding lane.
// cmax[tile]: widest row-slot class (1, 2, 4) among the tile's SNPs — a row of the tile is 64 * cmax ints, SNP `lane` slot i at lane * cmax + i;
// tbase[tile]: where the tile's RTlo rows start in the buffer; tf: the (tile, fs) pairs, fs < cmax[tile], LAST tiles first (the tile of the SNPs
// with >= 3 minor states — generic code, every unit listed, cmax 4 — is the critical path of the gathered GEMM and must not start last).
template <class RowsTo, class RowsFromSlot>
inline LoLayout lo_layout(int64_t nt, RowsTo rows_to, size_t n_slots, RowsFromSlot rows_from_slot, std::vector<int32_t> &cmax, std::vector<int64_t> &tbase,
                          std::vector<int32_t> &tf) {
    LoLayout lo;
    cmax.assign(n_slots / LO_TILE_SNPS, 1);
    tbase.assign(cmax.size(), 0);
    tf.clear();
    for (int64_t k = 0; k < nt; ++k) ++lo.n_lc[lo_class(rows_to(k))];
    int32_t uo = 0, rb = 0;
    for (int lc = 0; lc < 3; ++lc) {
        lo.uoff[lc] = uo;
        lo.rowbase[lc] = rb;
        uo += lo.n_lc[lc];
        rb += (int32_t)((((int64_t)lo.n_lc[lc] << lc) + LO_CHUNK_ROWS - 1) / LO_CHUNK_ROWS * LO_CHUNK_ROWS);
    }
    lo.RTlo = rb;
    lo.ntiles = (int32_t)cmax.size();
    for (size_t t = 0; t < n_slots; ++t) {
        const int nr = rows_from_slot(t);
        if (nr < 0) continue;
        const int cls = 1 << lo_class(nr);
        if (cls > cmax[t / LO_TILE_SNPS]) cmax[t / LO_TILE_SNPS] = cls;
    }
    int64_t tb = 0;
    for (size_t t = 0; t < cmax.size(); ++t) {
        tbase[t] = tb;
        tb += (int64_t)lo.RTlo * LO_TILE_SNPS * cmax[t];
        ++lo.n_tiles_cf[cmax[t] == 1 ? 0 : (cmax[t] == 2 ? 1 : 2)];
    }
    lo.glo_total = tb;
    for (size_t t = cmax.size(); t-- > 0;)
        for (int fs = 0; fs < cmax[t]; ++fs) {
            tf.push_back((int32_t)t);
            tf.push_back(fs);
        }
    lo.n_tf = (int32_t)(tf.size() / 2);
    return lo;
}

}  // namespace ldw

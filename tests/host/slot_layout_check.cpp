// Host check of the per-slot device buffers of a block's launch chain — the SAME descriptions the engine compiles (ldweaver_amd/csrc/ldw_slots.h:
// PacksLayout, UnitsLayout, PairsLayout, BinsLayout, MiniLayout, slot_geom_estimate).  For a list of block geometries it checks that the arrays of
// every buffer are pairwise disjoint, aligned and inside the byte count that is reserved, that a zeroed range covers exactly the arrays it is
// stated for, that no dimension shrinks a buffer when it grows, and that the geometry reserve_slot_buffers sizes the buffers for ahead of a pass
// is at least that of the benchmark's items.  Prints one line per geometry; exit code 0 iff nothing failed.
//   (tests/test_slot_layout_host.py builds it with g++ -O1 -std=c++17 and runs it)
#include <cstdio>
#include <string>
#include <vector>

#include "../../ldweaver_amd/csrc/ldw_slots.h"

using namespace ldw;

struct Arr {
    const char *name;
    size_t off, len, align;
    bool zeroed;
};
template <class T> Arr arr(const char *name, const Carve::Slot<T> &s, bool zeroed = false) {
    // 16 bytes for what k_zero4 clears and for the wide loads of the records, 8 for the 64-bit lists: every array at least 16.  (Carve steps by 256 bytes
    // today, so this holds by construction; the check is here for the day the step changes.)
    return Arr{name, s.off, s.len, std::max<size_t>(alignof(T), 16), zeroed};
}

static int failures = 0;
static void fail(const std::string &geom, const char *buf, const std::string &what) {
    ++failures;
    printf("FAIL [%s] %s: %s\n", geom.c_str(), buf, what.c_str());
}

// one buffer: its arrays as the layout names them, its byte count, and the range its zeroed() states (bytes 0: none)
static void check_buffer(const std::string &geom, const char *buf, const std::vector<Arr> &a, size_t bytes, const Carve &cv, Carve::Range z) {
    size_t sum = 0;
    for (size_t i = 0; i < a.size(); ++i) {
        sum += a[i].len;
        if (a[i].len == 0 || a[i].off + a[i].len > bytes) fail(geom, buf, std::string(a[i].name) + " is empty or leaves the buffer");
        if (a[i].off % a[i].align) fail(geom, buf, std::string(a[i].name) + " is misaligned");
        for (size_t j = i + 1; j < a.size(); ++j)
            if (a[i].off < a[j].off + a[j].len && a[j].off < a[i].off + a[i].len) fail(geom, buf, std::string(a[i].name) + " overlaps " + a[j].name);
    }
    if (sum != bytes) fail(geom, buf, "the arrays listed here do not add up to the buffer: one is missing from this check");
    // the zeroed range: every byte of it belongs to an array stated as zeroed, every such array lies inside it, and it is made of 16-byte pieces
    const size_t z0 = (size_t)(z.p - cv.base), z1 = z0 + z.bytes;
    size_t zsum = 0;
    for (const Arr &x : a) {
        const bool inside = x.off >= z0 && x.off + x.len <= z1, apart = x.off + x.len <= z0 || x.off >= z1;
        if (x.zeroed) zsum += x.len;
        if (x.zeroed && !inside) fail(geom, buf, std::string(x.name) + " is not covered by the zeroed range");
        if (!x.zeroed && !(apart || z.bytes == 0)) fail(geom, buf, std::string(x.name) + " is touched by the zeroed range");
    }
    if (zsum != z.bytes || z.bytes % 16 || z0 % 16 || (size_t)z.n16() * 16 != z.bytes) fail(geom, buf, "the zeroed range is not exactly its arrays");
}

struct Sizes {
    size_t packs, units, pairs, bins, mini;
    bool ge(const Sizes &o) const { return packs >= o.packs && units >= o.units && pairs >= o.pairs && bins >= o.bins && mini >= o.mini; }
};
static Sizes sizes_of(const SlotGeom &g, uint32_t pl_cap, uint32_t maybe_cap) {
    return Sizes{PacksLayout(g).bytes, UnitsLayout(g).bytes, PairsLayout(pl_cap, maybe_cap).bytes, BinsLayout(g).bytes, MiniLayout(g).bytes};
}

static void check_geom(const std::string &name, const SlotGeom &g) {
    static char mem[1];   // (a base to measure offsets from: nothing is read or written)
    const uint32_t pl_cap = pair_cap_of(g.nf, g.nt, g.nseg), maybe_cap = maybe_cap_of(g.RTpad, g.RFpad);
    {
        PacksLayout L(g);
        L.base = mem;
        check_buffer(name, "packs", {arr("cp", L.cp), arr("cp_hi", L.cp_hi), arr("rp", L.rp), arr("rp_hi", L.rp_hi), arr("rloc_f", L.rloc_f), arr("rloc_t", L.rloc_t)}, L.bytes,
                     L, Carve::Range{mem, 0});
    }
    {
        UnitsLayout L(g);
        L.base = mem;
        check_buffer(name, "units", {arr("counters", L.counters, true), arr("flat", L.flat), arr("tl", L.tl)}, L.bytes, L, L.zeroed());
        if ((size_t)(L.tile_cnt() - (unsigned int *)L.counters) != (size_t)UNIT_HDR_WORDS) fail(name, "units", "the per-tile counters do not start behind the header");
        if (L.flat.len < (size_t)(2 * L.list_stride) * 8) fail(name, "units", "the two flat lists do not fit their array");
        if (g.mixed && L.counters.len < (size_t)(UNIT_HDR_WORDS + 3 * g.nf_tiles) * 4) fail(name, "units", "the per-(tile, class) counters do not fit");
    }
    {
        PairsLayout L(pl_cap, maybe_cap);
        L.base = mem;
        check_buffer(name, "pairs", {arr("hdr", L.hdr, true), arr("lists", L.lists), arr("maybe", L.maybe)}, L.bytes, L, L.zeroed());
        if (L.hdr.off != 0) fail(name, "pairs", "the header does not open the buffer");
        if (L.lists.n != (size_t)PAIR_PATHS * PAIR_SHARDS * pl_cap || L.maybe.n != maybe_cap) fail(name, "pairs", "a list does not have its capacity");
        if (L.hdr.n != (size_t)PH_WORDS || PH_COUNT + PAIR_PATHS * PAIR_SHARDS > PH_MAYBE_OVER) fail(name, "pairs", "the header's words collide");
    }
    {
        BinsLayout L(g);
        L.base = mem;
        // (what phase 2 still reads — the slot flags — and everything k_build_packs has written by then must not be in the zeroed range)
        check_buffer(name, "bins",
                     {arr("bin_t", L.bin_t), arr("bin_f", L.bin_f), arr("rflag_t", L.rflag_t, true), arr("rflag_f", L.rflag_f, true), arr("n_live", L.n_live, true),
                      arr("sflag_t", L.sflag_t), arr("sflag_f", L.sflag_f), arr("tile_list", L.tile_list)},
                     L.bytes, L, L.zeroed());
        if (L.tile_list.n != (size_t)std::max<int64_t>(1, (g.RTpad / 64) * (g.RFpad / 64))) fail(name, "bins", "the tile list is not one word per 64 x 64 wave tile");
        if (L.bin_t.n != (size_t)g.RTpad || L.rflag_f.n != (size_t)g.RFpad || L.sflag_t.n != (size_t)g.nt || L.sflag_f.n != (size_t)g.nf_slots())
            fail(name, "bins", "a row or slot array does not have its side's count");
    }
    {
        MiniLayout L(g);
        L.base = mem;
        check_buffer(name, "mini", {arr("col", L.col), arr("row", L.row)}, L.bytes, L, Carve::Range{mem, 0});
    }
    // monotone: one dimension larger, no buffer smaller
    const Sizes s0 = sizes_of(g, pl_cap, maybe_cap);
    for (int dim = 0; dim < 9; ++dim) {
        SlotGeom h = g;
        uint32_t pc = pl_cap, mc = maybe_cap;
        if (dim == 0) h.nf += 1;
        if (dim == 1) h.nt += 1;
        if (dim == 2) h.RFpad += 128;
        if (dim == 3) h.RTpad += 128;
        if (dim == 4) h.nf_tiles += 1;
        if (dim == 5) h.nseg += 1;
        if (dim == 6) h.mixed = true;
        if (dim == 7) pc *= 2;
        if (dim == 8) mc += 1;
        if (dim < 6) {   // (the capacities follow the geometry)
            pc = pair_cap_of(h.nf, h.nt, h.nseg);
            mc = maybe_cap_of(h.RTpad, h.RFpad);
        }
        if (!sizes_of(h, pc, mc).ge(s0)) fail(name, "all", "dimension " + std::to_string(dim) + " grew and a buffer shrank");
    }
    printf("%-44s nf %6lld nt %6lld RF %6lld RT %6lld tiles %4lld nseg %d  packs %zu units %zu pairs %zu bins %zu mini %zu\n", name.c_str(), (long long)g.nf,
           (long long)g.nt, (long long)g.RFpad, (long long)g.RTpad, (long long)g.nf_tiles, g.nseg, s0.packs, s0.units, s0.pairs, s0.bins, s0.mini);
}

// A MODEL of the geometry build_side / build_perm_tiles give a block, written here: SNPs with one or two indicator rows only, `rho` rows per SNP on
// average; every row class starts on a 32-row boundary and the list is padded to 128 rows; every class of the from-side order is padded to whole tiles
// of 64.  What check_estimate proves about the C4 / C5 items is as good as this model (SNPs with three or four rows, or none, add up to two more
// tiles and 64 more rows, well inside the estimate's 512 rows and 6 tiles of slack).
static SlotGeom block_geom(int64_t nf, int64_t nt, double rho, int nseg) {
    auto rows = [rho](int64_t n) {
        const int64_t n2 = (int64_t)((rho - 1.0) * (double)n + 0.5), n1 = n - n2;
        const int64_t r = (n1 + 31) / 32 * 32 + (2 * n2 + 31) / 32 * 32;
        return std::max<int64_t>(128, (r + 127) / 128 * 128);
    };
    SlotGeom g;
    g.nf = nf;
    g.nt = nt;
    g.RFpad = rows(nf);
    g.RTpad = rows(nt);
    const int64_t n2 = (int64_t)((rho - 1.0) * (double)nf + 0.5);
    g.nf_tiles = std::max<int64_t>(1, (nf - n2 + 63) / 64 + (n2 + 63) / 64);
    g.nseg = nseg;
    return g;
}

// the ahead-of-time reserve against an item of the pass it was made for
static void check_estimate(const std::string &name, int64_t blk, int64_t nseg_max, const SlotGeom &item) {
    const SlotGeom e = slot_geom_estimate(blk, nseg_max);
    if (e.nf < item.nf || e.nt < item.nt || e.RFpad < item.RFpad || e.RTpad < item.RTpad || e.nf_tiles < item.nf_tiles || e.nseg < item.nseg)
        fail(name, "estimate", "a dimension of the estimated geometry is below the item's");
    const Sizes se = sizes_of(e, pair_cap_of(e.nf, e.nt, e.nseg), maybe_cap_of(e.RTpad, e.RFpad));
    const Sizes si = sizes_of(item, pair_cap_of(item.nf, item.nt, item.nseg), maybe_cap_of(item.RTpad, item.RFpad));
    if (!se.ge(si)) fail(name, "estimate", "a buffer reserved ahead of the pass is smaller than the item needs");
    printf("%-44s reserved ahead: packs %zu units %zu pairs %zu bins %zu mini %zu\n", name.c_str(), se.packs, se.units, se.pairs, se.bins, se.mini);
}

int main() {
    int n = 0;
    auto run = [&n](const std::string &name, SlotGeom g) {
        check_geom(name, g);
        g.mixed = true;
        check_geom(name + " (mixed)", g);
        ++n;
    };
    run("smallest block", SlotGeom{});
    run("ragged 65 x 1", SlotGeom{65, 1, 128, 128, 2, 0, false});
    run("ragged 1 x 257", SlotGeom{1, 257, 128, 384, 1, 0, false});
    run("no one-row SNP on the from side", block_geom(100, 100, 2.0, 0));
    run("span of 2", block_geom(500, 1000, 1.16, 2));
    run("span of LDW_SPAN_MAX", block_geom(500, 500 * LDW_SPAN_MAX, 1.16, LDW_SPAN_MAX));
    const SlotGeom c4d = block_geom(10000, 10000, 1.16, 0), c4s = block_geom(10000, 80000, 1.16, LDW_SPAN_MAX), c5 = block_geom(10000, 80000, 1.25, LDW_SPAN_MAX);
    run("C4 diagonal 10 000 x 10 000", c4d);
    run("C4 span 10 000 x 80 000", c4s);
    run("C5 block shape, 1.25 rows per SNP", c5);
    check_estimate("C4 diagonal against reserve(10 000, 8)", 10000, LDW_SPAN_MAX, c4d);
    check_estimate("C4 span against reserve(10 000, 8)", 10000, LDW_SPAN_MAX, c4s);
    check_estimate("C5 span against reserve(10 000, 8)", 10000, LDW_SPAN_MAX, c5);
    check_estimate("C4 diagonal against reserve(10 000, 1)", 10000, 1, c4d);
    printf("geometries %d  failures %d\n", n, failures);
    return failures == 0 ? 0 : 1;
}

// Host check of the low-limb geometry of the mixed-precision path — the SAME function the engine compiles (ldweaver_amd/csrc/ldw_lo_geom.h: lo_layout,
// which PrepWork::tiles and the test hook ldw_debug_lo_units both call).  Two checks:
//   * three block shapes whose values are worked out by hand below (the figures PrepWork::tiles gave for them when the arithmetic still stood there);
//   * the arithmetic as PrepWork::tiles had it before it moved into the header, kept here word for word (tiles_before), against lo_layout on those three
//     shapes and on a few hundred random ones: every number and every entry of cmax, tbase and tf.
// Prints one line per named shape; exit code 0 iff nothing failed.  (tests/test_lo_geom_host.py builds it with g++ -O1 -std=c++17 and runs it)
#include <cstdio>
#include <string>
#include <vector>

#include "../../ldweaver_amd/csrc/ldw_lo_geom.h"

using namespace ldw;

static int failures = 0;
static void fail(const std::string &shape, const std::string &what) {
    ++failures;
    printf("FAIL [%s] %s\n", shape.c_str(), what.c_str());
}

// a block: indicator rows of every to-side SNP, and of every lane of the from-tiles (-1: padding lane) — what row0 / perm give prep_block
struct Shape {
    std::vector<int> rows_to, rows_from;
};

struct Before {
    int32_t n_lc[3] = {0, 0, 0}, uoff[3] = {0, 0, 0}, rowbase[3] = {0, 0, 0}, RTlo = 0, ntiles = 0, n_tf = 0, n_tiles_cf[3] = {0, 0, 0};
    int64_t glo_total = 0;
    std::vector<int32_t> cmax, tf;
    std::vector<int64_t> tbase;
};

// PrepWork::tiles, as it was (its TILE = 128; pf[t] < 0 is the padding lane)
static Before tiles_before(const Shape &s) {
    Before lo;
    const int TILE = 128;
    auto class_of = [](int nrows) { return nrows <= 1 ? 0 : (nrows == 2 ? 1 : 2); };
    lo.cmax.assign(s.rows_from.size() / 64, 1);
    lo.tbase.assign(lo.cmax.size(), 0);
    for (size_t k = 0; k < s.rows_to.size(); ++k) ++lo.n_lc[class_of(s.rows_to[k])];
    int32_t uo = 0, rb = 0;
    for (int lc = 0; lc < 3; ++lc) {
        lo.uoff[lc] = uo;
        lo.rowbase[lc] = rb;
        uo += lo.n_lc[lc];
        rb += (int32_t)((((int64_t)lo.n_lc[lc] << lc) + TILE - 1) / TILE * TILE);
    }
    lo.RTlo = rb;
    lo.ntiles = (int32_t)lo.cmax.size();
    for (size_t t = 0; t < s.rows_from.size(); ++t) {
        if (s.rows_from[t] < 0) continue;
        const int cls = 1 << class_of(s.rows_from[t]);
        if (cls > lo.cmax[t / 64]) lo.cmax[t / 64] = cls;
    }
    int64_t tb = 0;
    for (size_t t = 0; t < lo.cmax.size(); ++t) {
        lo.tbase[t] = tb;
        tb += (int64_t)lo.RTlo * 64 * lo.cmax[t];
        ++lo.n_tiles_cf[lo.cmax[t] == 1 ? 0 : (lo.cmax[t] == 2 ? 1 : 2)];
    }
    lo.glo_total = tb;
    for (size_t t = lo.cmax.size(); t-- > 0;)
        for (int fs = 0; fs < lo.cmax[t]; ++fs) {
            lo.tf.push_back((int32_t)t);
            lo.tf.push_back(fs);
        }
    lo.n_tf = (int32_t)(lo.tf.size() / 2);
    return lo;
}

struct Now {
    LoLayout lo;
    std::vector<int32_t> cmax, tf;
    std::vector<int64_t> tbase;
};
static Now layout_now(const Shape &s) {
    Now n;
    n.tf.assign(5, 77);   // (stale content must not survive)
    n.lo = lo_layout(
        (int64_t)s.rows_to.size(), [&](int64_t k) { return s.rows_to[(size_t)k]; }, s.rows_from.size(), [&](size_t t) { return s.rows_from[t]; }, n.cmax, n.tbase, n.tf);
    return n;
}

static bool same(const Before &b, const Now &n) {
    bool ok = b.RTlo == n.lo.RTlo && b.ntiles == n.lo.ntiles && b.n_tf == n.lo.n_tf && b.glo_total == n.lo.glo_total && b.cmax == n.cmax && b.tbase == n.tbase && b.tf == n.tf;
    for (int k = 0; k < 3; ++k) ok = ok && b.n_lc[k] == n.lo.n_lc[k] && b.uoff[k] == n.lo.uoff[k] && b.rowbase[k] == n.lo.rowbase[k] && b.n_tiles_cf[k] == n.lo.n_tiles_cf[k];
    return ok;
}

struct Want {
    int32_t n_lc[3], uoff[3], rowbase[3], RTlo, n_tf, n_tiles_cf[3];
    int64_t glo_total;
    std::vector<int32_t> cmax, tf;
    std::vector<int64_t> tbase;
};

static void check_named(const std::string &name, const Shape &s, const Want &w) {
    const Now n = layout_now(s);
    bool ok = w.RTlo == n.lo.RTlo && w.n_tf == n.lo.n_tf && w.glo_total == n.lo.glo_total && w.cmax == n.cmax && w.tbase == n.tbase && w.tf == n.tf &&
              n.lo.ntiles == (int32_t)w.cmax.size();
    for (int k = 0; k < 3; ++k) ok = ok && w.n_lc[k] == n.lo.n_lc[k] && w.uoff[k] == n.lo.uoff[k] && w.rowbase[k] == n.lo.rowbase[k] && w.n_tiles_cf[k] == n.lo.n_tiles_cf[k];
    if (!ok) fail(name, "lo_layout does not give the hand-worked values");
    if (!same(tiles_before(s), n)) fail(name, "lo_layout differs from the arithmetic PrepWork::tiles had");
    printf("%-52s nt %5zu tiles %2d  n_lc %d %d %d  rowbase %d %d %d  RTlo %d  n_tf %d  glo %lld\n", name.c_str(), s.rows_to.size(), n.lo.ntiles, n.lo.n_lc[0], n.lo.n_lc[1],
           n.lo.n_lc[2], n.lo.rowbase[0], n.lo.rowbase[1], n.lo.rowbase[2], n.lo.RTlo, n.lo.n_tf, (long long)n.lo.glo_total);
}

static void add(std::vector<int> &v, int n, int rows) { v.insert(v.end(), (size_t)n, rows); }

int main() {
    int shapes = 0;
    {   // 200 / 70 / 3 to-side SNPs of 1 / 2 / 3 rows: class rows 200, 140, 12 -> 256, 256, 128.  Three from-tiles: one-row SNPs only; with a two-row SNP;
        // a three-row SNP and padding lanes.  Blocks of 640 rows x 64, 128, 256 ints.
        Shape s;
        add(s.rows_to, 200, 1), add(s.rows_to, 70, 2), add(s.rows_to, 3, 3);
        add(s.rows_from, 64, 1);
        add(s.rows_from, 63, 1), add(s.rows_from, 1, 2);
        add(s.rows_from, 1, 3), add(s.rows_from, 10, 1), add(s.rows_from, 53, -1);
        check_named("mixed classes, three tiles of cmax 1, 2, 4", s,
                    Want{{200, 70, 3}, {0, 200, 270}, {0, 256, 512}, 640, 7, {1, 1, 1}, 286720, {1, 2, 4}, {2, 0, 2, 1, 2, 2, 2, 3, 1, 0, 1, 1, 0, 0}, {0, 40960, 122880}});
        ++shapes;
    }
    {   // exactly one chunk of one-row SNPs, no other class (their row bases coincide); one tile that holds a single SNP without any row
        Shape s;
        add(s.rows_to, 128, 1);
        add(s.rows_from, 1, 0), add(s.rows_from, 63, -1);
        check_named("128 one-row SNPs, one lane without a row", s, Want{{128, 0, 0}, {0, 128, 128}, {0, 128, 128}, 128, 1, {1, 0, 0}, 8192, {1}, {0, 0}, {0}});
        ++shapes;
    }
    {   // 129 one-row SNPs (one past a chunk: 256 rows), 64 two-row (128 rows exactly), 33 four-row (132 -> 256); the SNPs without a row count as class 0
        Shape s;
        add(s.rows_to, 100, 1), add(s.rows_to, 64, 2), add(s.rows_to, 33, 4), add(s.rows_to, 27, 1), add(s.rows_to, 2, 0);
        add(s.rows_from, 1, 4), add(s.rows_from, 63, 2);
        add(s.rows_from, 20, -1), add(s.rows_from, 1, 3), add(s.rows_from, 43, -1);
        check_named("129 / 64 / 33 by class, two tiles of cmax 4", s,
                    Want{{129, 64, 33}, {0, 129, 193}, {0, 256, 384}, 640, 8, {0, 0, 2}, 327680, {4, 4}, {1, 0, 1, 1, 1, 2, 1, 3, 0, 0, 0, 1, 0, 2, 0, 3}, {0, 163840}});
        ++shapes;
    }
    // random shapes: any mix of row counts 0..4 on both sides, 1..9 tiles, padding lanes anywhere
    uint64_t x = 88172645463325252ull;
    auto rnd = [&x](uint64_t n) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return (int)(x % n);
    };
    int random_ok = 0;
    for (int it = 0; it < 400; ++it) {
        Shape s;
        const int nt = 1 + rnd(it % 4 == 0 ? 5000 : 300), ntiles = 1 + rnd(9), heavy = rnd(5);
        for (int k = 0; k < nt; ++k) s.rows_to.push_back(rnd(5) <= heavy ? 1 : rnd(5));
        for (int k = 0; k < 64 * ntiles; ++k) s.rows_from.push_back(rnd(4) == 0 ? -1 : (rnd(5) <= heavy ? 1 : rnd(5)));
        if (same(tiles_before(s), layout_now(s))) ++random_ok;
        else fail("random " + std::to_string(it), "lo_layout differs from the arithmetic PrepWork::tiles had");
    }
    printf("shapes %d  random %d  failures %d\n", shapes, random_ok, failures);
    return failures == 0 ? 0 : 1;
}

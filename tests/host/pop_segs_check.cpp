// Host check of the popcount segment tables and of the rule that picks a form of the exact pair sums — the SAME functions the engine compiles
// (ldweaver_amd/csrc/ldw_pairs.h: build_pop_segs, which prepare_apx_weights uploads from, and choose_pair_form, which launch_pair_sums launches by).
// Every expected value below is worked out by hand: the tables from the definition (weight classes = runs of equal positive weight along the
// positions, segments = their intersections with the 32-bit words), the forms from the rule as launch_pair_sums had it inline before it moved into
// the header.  Nothing expected is computed by the functions under test.
// Prints one line per case; exit code 0 iff nothing failed.  (tests/test_pop_segs_host.py builds it with g++ -O1 -std=c++17 -Wall -Werror and runs it)
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../ldweaver_amd/csrc/ldw_pairs.h"

using namespace ldw;

static int failures = 0, seg_cases = 0, form_cases = 0;
static void fail(const std::string &name, const std::string &what) {
    ++failures;
    printf("FAIL [%s] %s\n", name.c_str(), what.c_str());
}

struct Seg {
    uint32_t mask, flush;
    int64_t V;
};

// the tables of weights V (N of them, Npad positions) against the hand-worked segs / wbeg / counts; vpos and the cover of every word generically
static void check_segs(const char *name, const std::vector<int64_t> &V, int64_t Npad, const std::vector<Seg> &segs, const std::vector<uint32_t> &wbeg, int n_segs,
                       int n_classes) {
    ++seg_cases;
    const int64_t N = (int64_t)V.size();
    const PopSegTables T = build_pop_segs(V.data(), N, Npad);
    if (T.n_segs != n_segs) fail(name, "n_segs " + std::to_string(T.n_segs));
    if (T.n_classes != n_classes) fail(name, "n_classes " + std::to_string(T.n_classes));
    if (T.segs.size() != segs.size()) fail(name, "segs.size " + std::to_string(T.segs.size()));
    for (size_t i = 0; i < segs.size() && i < T.segs.size(); ++i)
        if (T.segs[i].mask != segs[i].mask || T.segs[i].flush != segs[i].flush || T.segs[i].V != segs[i].V) fail(name, "segs[" + std::to_string(i) + "]");
    if (T.wbeg.size() != wbeg.size() || (int64_t)wbeg.size() != Npad / 32 + 1) fail(name, "wbeg.size " + std::to_string(T.wbeg.size()));
    for (size_t w = 0; w < wbeg.size() && w < T.wbeg.size(); ++w)
        if ((uint32_t)T.wbeg[w] != wbeg[w]) fail(name, "wbeg[" + std::to_string(w) + "]");
    if ((int64_t)T.vpos.size() != Npad) fail(name, "vpos.size");
    for (int64_t p = 0; p < Npad && p < (int64_t)T.vpos.size(); ++p)
        if (T.vpos[(size_t)p] != (p < N ? V[(size_t)p] : 0)) fail(name, "vpos[" + std::to_string(p) + "]");
    // every word: its masks are disjoint and cover exactly the positions below N with a positive weight
    for (int64_t w = 0; w + 1 < (int64_t)T.wbeg.size(); ++w) {
        uint32_t want = 0, got = 0;
        for (int b = 0; b < 32; ++b)
            if (32 * w + b < N && V[(size_t)(32 * w + b)] > 0) want |= 1u << b;
        const int s0 = T.wbeg[(size_t)w] & 0x7FFFFFFF, s1 = T.wbeg[(size_t)w + 1] & 0x7FFFFFFF;
        for (int s = s0; s < s1 && s < T.n_segs; ++s) {
            if (got & T.segs[(size_t)s].mask) fail(name, "masks of word " + std::to_string(w) + " overlap");
            got |= T.segs[(size_t)s].mask;
        }
        if (got != want) fail(name, "cover of word " + std::to_string(w));
    }
    printf("segs [%s] done\n", name);
}

// rc != LDW_OK: only rc is compared
static void check_form(const char *name, int nwords, int nseg, bool have_vpos, bool want_wave, bool bits_off, int requested, int rc, int form, int seg_in_lds,
                       size_t lds, bool lds160) {
    ++form_cases;
    const PairFormChoice ch = choose_pair_form(nwords, nseg, have_vpos, want_wave, bits_off, requested);
    if (ch.rc != rc) fail(name, "rc " + std::to_string(ch.rc));
    if (rc != LDW_OK) {
        if (ch.msg[0] == 0) fail(name, "no message");
    } else if (ch.form != form || ch.seg_in_lds != seg_in_lds || ch.lds != lds || ch.lds160 != lds160) {
        fail(name, "form " + std::to_string(ch.form) + " seg_in_lds " + std::to_string(ch.seg_in_lds) + " lds " + std::to_string(ch.lds) + " lds160 " +
                       std::to_string((int)ch.lds160));
    }
    printf("form [%s] done\n", name);
}

int main() {
    const uint32_t FULL = 0xFFFFFFFFu, B31 = 0x80000000u;
    // ---- the segment tables
    // N = 33, one class: word 0 is one full mask that does not end the class (bit 31 of wbeg), word 1 holds bit 0 and ends it, words 2 and 3 are empty
    check_segs("N33 one class", std::vector<int64_t>(33, 7), 128, {{FULL, 0, 7}, {0x1u, 1, 7}}, {B31 | 0u, 1, 2, 2, 2}, 2, 1);
    {   // a class border in the middle of word 0: positions 0..9 weigh 3, 10..39 weigh 5 (the second class goes on into word 1)
        std::vector<int64_t> V(40, 5);
        for (int p = 0; p < 10; ++p) V[(size_t)p] = 3;
        check_segs("border inside a word", V, 128, {{0x3FFu, 1, 3}, {0xFFFFFC00u, 0, 5}, {0xFFu, 1, 5}}, {0, 2, 3, 3, 3}, 3, 2);
    }
    {   // a class that ends exactly at a word's last bit: full mask, flush 1, bit 31 clear
        std::vector<int64_t> V(64, 9);
        for (int p = 0; p < 32; ++p) V[(size_t)p] = 2;
        check_segs("class ends with its word", V, 128, {{FULL, 1, 2}, {FULL, 1, 9}}, {0, 1, 2, 2, 2}, 2, 2);
    }
    {   // a run of zero weights between two classes: no segment, not counted
        std::vector<int64_t> V(20, 0);
        for (int p = 0; p < 5; ++p) V[(size_t)p] = 4;
        for (int p = 12; p < 20; ++p) V[(size_t)p] = 6;
        check_segs("zero run between classes", V, 128, {{0x1Fu, 1, 4}, {0xFF000u, 1, 6}}, {0, 2, 2, 2, 2}, 2, 2);
    }
    // N a multiple of 32: the class ends with word 0
    check_segs("N32 one class", std::vector<int64_t>(32, 11), 128, {{FULL, 1, 11}}, {0, 1, 1, 1, 1}, 1, 1);
    // N a multiple of 128 = Npad: three full words that do not end the class, the fourth ends it
    check_segs("N128 one class", std::vector<int64_t>(128, 1), 128, {{FULL, 0, 1}, {FULL, 0, 1}, {FULL, 0, 1}, {FULL, 1, 1}}, {B31 | 0u, B31 | 1u, B31 | 2u, 3, 4}, 4, 1);
    {   // 64 distinct weights over 64 positions: a class per position, 32 segments per word
        std::vector<int64_t> V(64);
        std::vector<Seg> segs;
        for (int p = 0; p < 64; ++p) {
            V[(size_t)p] = p + 1;
            segs.push_back(Seg{1u << (p % 32), 1, (int64_t)p + 1});
        }
        check_segs("64 distinct weights", V, 128, segs, {0, 32, 64, 64, 64}, 64, 64);
    }
    // all weights zero: the placeholder record, count 0
    check_segs("all zero", std::vector<int64_t>(10, 0), 128, {{0, 0, 0}}, {0, 0, 0, 0, 0}, 0, 0);

    // ---- the form rule.  Segment tables of (nwords, nseg): (nwords + 4) * 4 rounded up to 16, plus 16 bytes per record; the bit walk's table:
    // 256 bytes per word, the words rounded up to 32.
    const int Q = PAIR_FORM_QUARTER, WL = PAIR_FORM_WAVE_LDS, WG = PAIR_FORM_WAVE_GLOBAL, BW = PAIR_FORM_BITS;
    // C4-like: 160 words, 211 records: 656 + 3376 = 4032 B; few classes
    check_form("default", 160, 211, true, false, false, 0, LDW_OK, Q, 1, 4032, false);
    check_form("want_wave", 160, 211, true, true, false, 0, LDW_OK, WL, 1, 4032, false);
    // the 60 000 B gate (bit walk off, so that the class-wise forms show it): 160 words, 3709 records = 656 + 59 344 = 60 000 B; one record more = 60 016 B
    check_form("60000 B, quarter", 160, 3709, true, false, true, 0, LDW_OK, Q, 1, 60000, false);
    check_form("60000 B, wave", 160, 3709, true, true, true, 0, LDW_OK, WL, 1, 60000, false);
    check_form("60016 B, global", 160, 3710, true, false, true, 0, LDW_OK, WG, 0, 0, false);
    check_form("60016 B, global, want_wave", 160, 3710, true, true, true, 0, LDW_OK, WG, 0, 0, false);
    check_form("60016 B, no vpos", 160, 3710, false, false, false, 0, LDW_OK, WG, 0, 0, false);
    // ... and with the bit walk on, both sides have many classes: 160 words -> 32 * 160 * 8 = 40 960 B; seg_in_lds still says whether the tables fit
    check_form("60000 B, bits", 160, 3709, true, false, false, 0, LDW_OK, BW, 1, 40960, false);
    check_form("60016 B, bits", 160, 3710, true, false, false, 0, LDW_OK, BW, 0, 40960, false);
    // the class-count gate: nseg = 8 * nwords - 1 = 1279 (656 + 20 464 = 21 120 B) and 8 * nwords = 1280 (21 136 B)
    check_form("1279 records", 160, 1279, true, false, false, 0, LDW_OK, Q, 1, 21120, false);
    check_form("1280 records", 160, 1280, true, false, false, 0, LDW_OK, BW, 1, 40960, false);
    check_form("1280 records, want_wave", 160, 1280, true, true, false, 0, LDW_OK, BW, 1, 40960, false);
    check_form("1280 records, bits_off", 160, 1280, true, false, true, 0, LDW_OK, Q, 1, 21136, false);
    check_form("1280 records, bits_off, want_wave", 160, 1280, true, true, true, 0, LDW_OK, WL, 1, 21136, false);
    check_form("1280 records, no vpos", 160, 1280, false, false, false, 0, LDW_OK, Q, 1, 21136, false);
    // the bit walk's table at 64 KB (256 words: 65 536 B) and one stride step above (288 words: 73 728 B); nseg = 8 * nwords, tables 33 808 / 38 032 B
    check_form("bits 64 KB", 256, 2048, true, false, false, 0, LDW_OK, BW, 1, 65536, false);
    check_form("bits 72 KB", 288, 2304, true, false, false, 0, LDW_OK, BW, 1, 73728, true);
    // at 160 KB (640 words: 163 840 B) and one stride step above (672 words: 172 032 B); nseg = 8 * nwords, tables 84 496 / 88 720 B: not in LDS
    check_form("bits 160 KB", 640, 5120, true, false, false, 0, LDW_OK, BW, 0, 163840, true);
    check_form("bits 168 KB", 672, 5376, true, false, false, 0, LDW_OK, WG, 0, 0, false);
    // requested forms; the switches do not bear on them
    check_form("ask 1", 160, 211, true, true, true, 1, LDW_OK, Q, 1, 4032, false);
    check_form("ask 2", 160, 211, true, false, false, 2, LDW_OK, WL, 1, 4032, false);
    check_form("ask 3", 160, 211, true, false, false, 3, LDW_OK, WG, 0, 0, false);
    check_form("ask 4", 160, 211, true, false, true, 4, LDW_OK, BW, 1, 40960, false);
    check_form("ask 4, no vpos", 160, 211, false, false, false, 4, LDW_ERR_STATE, 0, 0, 0, false);
    check_form("ask 1, 60000 B", 160, 3709, true, false, false, 1, LDW_OK, Q, 1, 60000, false);
    check_form("ask 1, 60016 B", 160, 3710, true, false, false, 1, LDW_ERR_STATE, 0, 0, 0, false);
    check_form("ask 2, 60016 B", 160, 3710, true, false, false, 2, LDW_ERR_STATE, 0, 0, 0, false);
    check_form("ask 3, 60016 B", 160, 3710, true, false, false, 3, LDW_OK, WG, 0, 0, false);
    check_form("ask 4, 60016 B", 160, 3710, true, false, false, 4, LDW_OK, BW, 0, 40960, false);
    check_form("ask 4, 160 KB", 640, 5120, true, false, false, 4, LDW_OK, BW, 0, 163840, true);
    check_form("ask 4, 168 KB", 672, 5376, true, false, false, 4, LDW_ERR_STATE, 0, 0, 0, false);
    check_form("ask 3, 168 KB", 672, 5376, true, false, false, 3, LDW_OK, WG, 0, 0, false);
    check_form("ask 5", 160, 211, true, false, false, 5, LDW_ERR_ARG, 0, 0, 0, false);
    check_form("ask -1", 160, 211, true, false, false, -1, LDW_ERR_ARG, 0, 0, 0, false);

    printf("segs %d forms %d failures %d\n", seg_cases, form_cases, failures);
    return failures ? 1 : 0;
}

// Exact joint sums of the listed long-range pairs (ldw_pairs.hip), shared declarations.
//
// What the screen of the approximate path (ldw_apx.h) lists gets EXACT joint sums.  Long-range candidates (one pair in a few thousand) are
// listed PAIR by pair and need no GEMM at all: sum_s V_s x_s y_s = sum over 32-bit words and weight classes of V_class popcount(x & y & class
// mask), a quarter-wave per pair, four pairs per persistent wave, a lane holding two words of every 32 (k_pair_sums_q; k_pair_sums, a wave per
// pair with lane = word, where the segment tables do not fit LDS or LDW_PAIR_WAVE=1; k_pair_sums_bits, a walk over the set bits, for weightings
// with many classes), then the fp64 MI (k_pair_mi).
//
// The first part — the popcount segment tables of a weighting and the rule that picks a form — is plain C++ on the host:
// tests/host/pop_segs_check.cpp reads this header with g++ (tests/test_pop_segs_host.py).  The launchers follow under __HIPCC__.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/ldweaver_amd.h"

namespace ldw {

// one (32-bit word, weight class) intersection of the position axis
struct PopSeg {
    uint32_t mask;    // bits of the word that belong to the class
    uint32_t flush;   // 1: last segment of its class: fold the class count into the 64-bit sums with weight V
    int64_t V;        // fixed-point weight of the class
};

// The segment tables of a weighting, as they are uploaded (ApxWeights::pop_segs, pop_wbeg, pop_vpos).
struct PopSegTables {
    std::vector<PopSeg> segs;    // by word, then by position; ONE placeholder record {0, 0, 0} when there is no segment (n_segs stays 0)
    std::vector<int32_t> wbeg;   // [Npad / 32 + 1] first segment of every word; bit 31: the word is ONE full segment that does not end its class
                                 // (k_units_pop reads no segment record for it)
    std::vector<int64_t> vpos;   // [Npad] weight of every position, 0 in the padding (k_pair_sums_bits)
    int n_segs = 0, n_classes = 0;
};

// Vp[0 .. N): fixed-point weights by POSITION; Npad: a multiple of 32, >= N.  Weight classes = runs of equal V along the positions (a run of
// zeros is no class); segments = (32-bit word, class) intersections.
inline PopSegTables build_pop_segs(const int64_t *Vp, int64_t N, int64_t Npad) {
    PopSegTables T;
    T.wbeg.assign((size_t)(Npad / 32) + 1, 0);
    T.vpos.assign((size_t)Npad, 0);
    std::copy(Vp, Vp + N, T.vpos.begin());
    std::vector<std::vector<PopSeg>> per_word((size_t)(Npad / 32));
    for (int64_t p0 = 0; p0 < N;) {
        int64_t p1 = p0 + 1;
        while (p1 < N && Vp[p1] == Vp[p0]) ++p1;
        if (Vp[p0] > 0) {
            ++T.n_classes;
            for (int64_t w = p0 / 32; w <= (p1 - 1) / 32; ++w) {
                const int64_t lo = std::max<int64_t>(p0, w * 32) - w * 32, hi = std::min<int64_t>(p1, w * 32 + 32) - w * 32;   // bits [lo, hi)
                const uint32_t mask = (hi >= 32 ? 0xFFFFFFFFu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u);
                per_word[(size_t)w].push_back(PopSeg{mask, w == (p1 - 1) / 32 ? 1u : 0u, Vp[p0]});
            }
        }
        p0 = p1;
    }
    for (size_t w = 0; w < per_word.size(); ++w) {
        T.wbeg[w] = (int32_t)T.segs.size();
        if (per_word[w].size() == 1 && per_word[w][0].mask == 0xFFFFFFFFu && !per_word[w][0].flush) T.wbeg[w] |= (int32_t)0x80000000;
        for (auto &s : per_word[w]) T.segs.push_back(s);
    }
    T.wbeg[per_word.size()] = (int32_t)T.segs.size();
    T.n_segs = (int)T.segs.size();
    if (T.segs.empty()) T.segs.push_back(PopSeg{0, 0, 0});
    return T;
}

// Dynamic LDS of the sum kernels.  The class-wise forms: wbeg[nwords + 1] (padded to 16 bytes), then nseg segment records — with nseg = 0, where the
// records start.  The bit walk: the weight of every position as [bit][word], the words padded to a multiple of 32 (pair_bits_stride).
constexpr size_t pop_seg_lds_bytes(int nwords, int nseg) { return (((size_t)nwords + 4) * 4 + 15) / 16 * 16 + (size_t)nseg * sizeof(PopSeg); }
constexpr int pair_bits_stride(int nwords) { return (nwords + 31) / 32 * 32; }
constexpr size_t pair_bits_lds_bytes(int nwords) { return (size_t)32 * pair_bits_stride(nwords) * 8; }
constexpr size_t PAIR_SEG_LDS_MAX = 60000;          // the segment tables are staged in LDS up to here, else read from global memory
constexpr size_t PAIR_BITS_LDS_MAX = 160 * 1024;    // the bit walk runs up to here (above 64 KB with the dynamic-LDS attribute)

// The forms of the exact pair sums (the numbers of ldw_debug_pair_sums): a quarter-wave per pair (k_pair_sums_q), a wave per pair with the segment
// tables in LDS / in global memory (k_pair_sums), the bit walk (k_pair_sums_bits).
enum PairForm : int { PAIR_FORM_AUTO = 0, PAIR_FORM_QUARTER = 1, PAIR_FORM_WAVE_LDS = 2, PAIR_FORM_WAVE_GLOBAL = 3, PAIR_FORM_BITS = 4 };

struct PairFormChoice {
    int rc = LDW_OK;       // LDW_ERR_ARG / LDW_ERR_STATE: the requested form cannot run (msg says why), nothing else is set
    int form = 0;          // 1..4
    int seg_in_lds = 0;    // PairArgs::seg_in_lds
    size_t lds = 0;        // dynamic LDS of the form's two launches
    bool lds160 = false;   // the bit walk above 64 KB
    char msg[160] = "";
};

// Which form runs for rows of nwords 32-bit words and nseg segment records.  have_vpos: the per-position weights are on the device; want_wave:
// LDW_PAIR_WAVE; bits_off: LDW_NO_PAIR_BITS; requested_form: PAIR_FORM_AUTO = the product's choice, else that form or the error.
// (Which form: the class-wise one costs a popcount per SEGMENT — 1.3 segments per word with C4's 57 clonal classes —, the bit walk an LDS read per
// co-occurring position; from ~8 segments per word on, i.e. weightings whose classes are a few sequences each, the bits are fewer than the segments.
// The bit walk's table is 256 B per word of a row: 40 KB at N = 5120, 80 KB at 10 240; beyond 160 KB — N > 20 480 — the class-wise kernel reads its
// tables from global memory.)
inline PairFormChoice choose_pair_form(int nwords, int nseg, bool have_vpos, bool want_wave, bool bits_off, int requested_form) {
    PairFormChoice ch;
    const size_t lds = pop_seg_lds_bytes(nwords, nseg), lds_bits = pair_bits_lds_bytes(nwords);
    const bool fits = lds <= PAIR_SEG_LDS_MAX;
    const bool bits_can = lds_bits <= PAIR_BITS_LDS_MAX && have_vpos;
    auto refuse = [&ch](int rc, const char *fmt, auto... args) {
        ch.rc = rc;
        snprintf(ch.msg, sizeof(ch.msg), fmt, args...);
        return ch;
    };
    int form = requested_form;
    if (form == PAIR_FORM_AUTO) {
        const bool many_classes = !fits || nseg >= 8 * nwords;
        if (many_classes && !bits_off && bits_can) form = PAIR_FORM_BITS;
        else if (fits && !want_wave) form = PAIR_FORM_QUARTER;
        else form = fits ? PAIR_FORM_WAVE_LDS : PAIR_FORM_WAVE_GLOBAL;
    } else if (form < PAIR_FORM_QUARTER || form > PAIR_FORM_BITS) {
        return refuse(LDW_ERR_ARG, "pair sums: form %d outside 0..4", form);
    } else if (!fits && (form == PAIR_FORM_QUARTER || form == PAIR_FORM_WAVE_LDS)) {
        return refuse(LDW_ERR_STATE, "pair sums: form %d needs the popcount segment tables in LDS (%zu B > 60000 B)", form, lds);
    } else if (form == PAIR_FORM_BITS && !bits_can) {
        return refuse(LDW_ERR_STATE, "pair sums: the bit walk needs a per-position weight table of at most 160 KB of LDS (%zu B)", lds_bits);
    }
    ch.form = form;
    ch.seg_in_lds = (fits && form != PAIR_FORM_WAVE_GLOBAL) ? 1 : 0;
    ch.lds = form == PAIR_FORM_BITS ? lds_bits : (ch.seg_in_lds ? lds : 0);
    ch.lds160 = form == PAIR_FORM_BITS && lds_bits > 64 * 1024;
    return ch;
}

}  // namespace ldw

#if defined(__HIPCC__)
#include "ldw_internal.h"
#include "ldw_epi.h"

namespace ldw {

struct PairArgs {
    const uint64_t *Mbits;
    int64_t KW;
    int nwords, path, nseg;      // 32-bit words per row; segment records
    int seg_in_lds;              // the segment tables fit the workgroup's LDS (else they are read from global memory)
    const PopSeg *segs;
    const int32_t *wbeg, *row0;
    int32_t zero_row;
    int64_t *sums;
    EpiArgs A;
    unsigned long long *ghist;
};

struct PairSumsRan {
    int form = 0;          // the form that was launched (1..4)
    bool lds160 = false;   // the bit walk with the 160-KB dynamic-LDS attribute
};
// The sums alone, sums[(list * A.pl_cap + i) * 16 + j * 4 + i'] of the lists A.pl_pairs / A.pl_n / A.pl_cap (nothing else of A is read): form
// PAIR_FORM_AUTO = the product's choice, else that form or LDW_ERR_STATE where it cannot run; grid_wgs 0 = the product's grid, else gridDim.x of
// both launches (the quarter-wave kernel: the whole grid of a path; the others: workgroups per list).  Counts nothing.
int launch_pair_sums(ldw_ctx *c, const EpiArgs &A, int64_t *sums, hipStream_t st, int form, int grid_wgs, PairSumsRan *ran);
// the pair lists of A (filled by the approximate screen): exact sums (launch_pair_sums(.., PAIR_FORM_AUTO, 0)), fp64 MI, emission
int launch_pairs_exact(ldw_ctx *c, const EpiArgs &A, unsigned long long *ghist, int64_t *sums, hipStream_t st);

}  // namespace ldw
#endif

// SnpEff step of perform_snpEff_annotations (R/SnpEffAnnotations.R:29-103) on the device: the coding effect of every annotated SNP and the
// join of the per-SNP annotation onto the links with the top-hit selection (add_annotations_to_links :324-391, detect_top_hits :393-403).
//
//   ldw_annot_snps  : k_annot_snp, one lane per SNP: the SNP is stabbed into the CDS segments (binary search over the starts with a running
//                     maximum of the ends, as k_cds_span), every (allele, covering feature) pair is translated with codon table 11 from the
//                     reference on the device, and the highest-impact pair is kept; a SNP outside every segment takes the nearest feature within
//                     5000 bp (up/downstream) or its two neighbours (intergenic).  One fixed record of LDW_ANNOT_REC int32 per SNP; the host
//                     renders the strings.  The rule table is DESIGN.md 19.
//   ldw_annot_map   : every link end to its SNP (binary search over the sorted positions), the used SNPs marked, a scan over the sorted
//                     positions gives every used SNP its annotation row (= rank among the distinct link positions), kept for ldw_annot_links.
//   ldw_annot_links : an order-preserving key of srp / MI (decreasing, NaN last, stable: R's order) through the radix sort with the row index,
//                     then per sorted link the rows, the code pair and the top-hit test, and a scan that compacts the first max_tophits passes.
//
// Every pass is a grid-stride loop over a bounded grid with int64 indices; all global writes are vector stores or vector atomics.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "ldw_work.h"
#include "ldw_dev.h"

using namespace ldw;

namespace {

constexpr int64_t UPDOWN = 5000;   // snpEff's default up/downstream length

// effects (ldweaver_amd/annotate.py EFFECTS holds the names in this order) and impacts
enum : int32_t {
    E_NONE = 0, E_START_LOST, E_STOP_GAINED, E_STOP_LOST, E_MISSENSE, E_START_RETAINED, E_SYNONYMOUS, E_STOP_RETAINED, E_CODING, E_UPSTREAM,
    E_DOWNSTREAM, E_INTERGENIC
};
__device__ __forceinline__ int32_t impact_of(int32_t e) {
    return e <= E_STOP_LOST ? 3 : e == E_MISSENSE ? 2 : e <= E_STOP_RETAINED ? 1 : 0;
}

// T C A G order: the standard code, which table 11 shares for every amino acid
__constant__ char AA_TCAG[65] = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";

__device__ __forceinline__ int tcag(char b) { return b == 'T' ? 0 : b == 'C' ? 1 : b == 'A' ? 2 : b == 'G' ? 3 : -1; }
__device__ __forceinline__ char upper(char b) { return (b >= 'a' && b <= 'z') ? (char)(b - 32) : b; }
__device__ __forceinline__ char comp(char b) {
    return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : b;
}
// table 11 start codons: ATG GTG TTG CTG ATT ATC ATA
__device__ __forceinline__ bool is_start(const char *k) {
    if (k[0] == 'A' && k[1] == 'T') return k[2] == 'G' || k[2] == 'T' || k[2] == 'C' || k[2] == 'A';
    return k[1] == 'T' && k[2] == 'G' && (k[0] == 'G' || k[0] == 'T' || k[0] == 'C');
}
__device__ __forceinline__ char translate(const char *k) {
    const int a = tcag(k[0]), b = tcag(k[1]), d = tcag(k[2]);
    return (a < 0 || b < 0 || d < 0) ? 0 : AA_TCAG[a * 16 + b * 4 + d];
}

// The device image of the feature table (one int32 array, built by the host half of ldw_annot_snps):
//   F  [nfeat][8]  lo, hi (extent), strand (+1 / -1), first segment, segments, rank (order of (lo, file index)), spliced length, 0
//   S  [nseg][4]   lo, hi, coding offset of the segment's first coding base, feature   (per feature contiguous, in coding order)
//   stl, stm, sti [nseg]   segments by lo: lo, running maximum of hi, segment
//   bsl, bsf [nfeat]       features by (lo, rank): lo, feature
//   beh, bef [nfeat]       features by (hi, rank): hi, feature
struct Tables {
    const int32_t *F, *S, *stl, *stm, *sti, *bsl, *bsf, *beh, *bef;
    int64_t nfeat, nseg;
};

// the genome position (1-based) of coding base cc (0-based) of feature f
__device__ __forceinline__ int64_t coding_to_genome(const Tables &t, int32_t f, int64_t cc) {
    const int32_t s0 = t.F[f * 8 + 3], ns = t.F[f * 8 + 4], strand = t.F[f * 8 + 2];
    for (int32_t s = s0; s < s0 + ns; ++s) {
        const int64_t lo = t.S[s * 4], hi = t.S[s * 4 + 1], cum = t.S[s * 4 + 2];
        if (cc >= cum && cc < cum + (hi - lo + 1)) return strand > 0 ? lo + (cc - cum) : hi - (cc - cum);
    }
    return -1;
}

// record words (LDW_ANNOT_REC = 12): effect, impact, feature (intergenic: left or -1), right feature (intergenic) or -1, c (coding) or distance
// (up/down), codon number k, ref base, alt base (coding strand for coding and up/down SNPs, + strand for intergenic; 0: no A/C/G/T allele),
// ref amino acid, alt amino acid ('*' stop; 0: none), allele (0..3 = A C G T, -1 none), 0
__global__ __launch_bounds__(256) void k_annot_snp(Tables t, const char *__restrict__ ref, int64_t g, const int32_t *__restrict__ pos,
                                                   const uint8_t *__restrict__ alt, int64_t n, int32_t *__restrict__ rec) {
    const char ACGT[4] = {'A', 'C', 'G', 'T'};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t p = pos[i];
        const uint32_t m = alt[i] & 15u;
        int32_t r[12] = {E_NONE, 0, -1, -1, 0, 0, 0, 0, 0, 0, -1, 0};
        const char refp = upper(ref[p - 1]);
        // ---- coding: every segment that holds p
        int best_imp = -1, best_a = 99, best_rank = 0x7fffffff;
        int64_t best_c = 0;
        int32_t cov_f = -1, cov_rank = 0x7fffffff;
        for (int64_t j = upper_bound_dev<int64_t>(t.stl, t.nseg, p) - 1; j >= 0 && t.stm[j] >= p; --j) {
            const int32_t s = t.sti[j];
            if (t.S[s * 4 + 1] < p) continue;
            const int32_t f = t.S[s * 4 + 3];
            const int32_t strand = t.F[f * 8 + 2], rank = t.F[f * 8 + 5];
            const int64_t len = t.F[f * 8 + 6];
            const int64_t cc = t.S[s * 4 + 2] + (strand > 0 ? p - t.S[s * 4] : t.S[s * 4 + 1] - p);   // 0-based
            if (rank < cov_rank) { cov_rank = rank; cov_f = f; }
            const int64_t k = cc / 3 + 1, at = cc % 3;
            const bool complete = 3 * k <= len;
            char kr[3] = {0, 0, 0};
            if (complete)
                for (int q = 0; q < 3; ++q) kr[q] = upper(ref[coding_to_genome(t, f, 3 * (k - 1) + q) - 1]), kr[q] = strand > 0 ? kr[q] : comp(kr[q]);
            const char rb = strand > 0 ? refp : comp(refp);
            for (int a = 0; a < 4; ++a) {
                if (!((m >> a) & 1u)) continue;
                const char ab = strand > 0 ? ACGT[a] : comp(ACGT[a]);
                char ka[3] = {kr[0], kr[1], kr[2]};
                ka[at] = ab;
                int32_t e;
                char ra = 0, aa = 0;
                if (k == 1 && complete && is_start(kr)) {
                    ra = 'M';
                    e = is_start(ka) ? E_START_RETAINED : E_START_LOST;
                    aa = e == E_START_RETAINED ? 'M' : 0;
                } else if (!complete || translate(kr) == 0 || translate(ka) == 0) {
                    e = E_CODING;
                } else {
                    ra = translate(kr);
                    aa = translate(ka);
                    e = ra == aa ? (ra == '*' ? E_STOP_RETAINED : E_SYNONYMOUS) : aa == '*' ? E_STOP_GAINED : ra == '*' ? E_STOP_LOST : E_MISSENSE;
                }
                const int imp = impact_of(e);
                const bool better = imp > best_imp ||
                                    (imp == best_imp && (a < best_a || (a == best_a && (rank < best_rank || (rank == best_rank && cc + 1 < best_c)))));
                if (better) {
                    best_imp = imp, best_a = a, best_rank = rank, best_c = cc + 1;
                    r[0] = e, r[1] = imp, r[2] = f, r[4] = (int32_t)(cc + 1), r[5] = (int32_t)k, r[6] = rb, r[7] = ab, r[8] = ra, r[9] = aa, r[10] = a;
                }
            }
        }
        if (cov_f >= 0 && r[0] == E_NONE) {   // covered, but no A/C/G/T allele
            r[0] = E_CODING, r[1] = 0, r[2] = cov_f;
        }
        if (cov_f < 0) {
            // ---- non-coding: the nearest feature end on each side (features whose extent holds p are on neither side)
            const int64_t jr = upper_bound_dev<int64_t>(t.bsl, t.nfeat, p);              // first feature (by lo) that starts after p
            const int64_t jl = lower_bound_dev<int64_t>(t.beh, t.nfeat, p) - 1;          // last feature (by hi) that ends before p
            const int64_t dr = jr < t.nfeat ? t.bsl[jr] - p : INT64_MAX, dl = jl >= 0 ? p - t.beh[jl] : INT64_MAX;
            const int64_t d = dr < dl ? dr : dl;
            int a0 = -1;
            for (int a = 3; a >= 0; --a)
                if ((m >> a) & 1u) a0 = a;
            if (d <= UPDOWN) {
                int32_t bf = -1, bkey = 0x7fffffff;   // key: (downstream, rank)
                if (dr == d)
                    for (int64_t j = jr; j < t.nfeat && t.bsl[j] == t.bsl[jr]; ++j) {
                        const int32_t f = t.bsf[j], up = t.F[f * 8 + 2] > 0 ? 0 : 1;
                        const int32_t key = up * (int32_t)t.nfeat + t.F[f * 8 + 5];
                        if (key < bkey) bkey = key, bf = f;
                    }
                if (dl == d)
                    for (int64_t j = jl; j >= 0 && t.beh[j] == t.beh[jl]; --j) {
                        const int32_t f = t.bef[j], up = t.F[f * 8 + 2] < 0 ? 0 : 1;
                        const int32_t key = up * (int32_t)t.nfeat + t.F[f * 8 + 5];
                        if (key < bkey) bkey = key, bf = f;
                    }
                const bool up = bkey < (int32_t)t.nfeat;
                const int32_t strand = t.F[bf * 8 + 2];
                r[0] = up ? E_UPSTREAM : E_DOWNSTREAM, r[1] = 0, r[2] = bf, r[4] = (int32_t)d;
                r[6] = strand > 0 ? refp : comp(refp);
                r[7] = a0 < 0 ? 0 : (strand > 0 ? ACGT[a0] : comp(ACGT[a0]));
            } else {
                int32_t lf = -1, rf = -1;
                if (jr < t.nfeat) rf = t.bsf[jr];   // (by (lo, rank): the first of its run has the lowest rank)
                if (jl >= 0) {
                    int32_t bk = 0x7fffffff;
                    for (int64_t j = jl; j >= 0 && t.beh[j] == t.beh[jl]; --j)
                        if (t.F[t.bef[j] * 8 + 5] < bk) bk = t.F[t.bef[j] * 8 + 5], lf = t.bef[j];
                }
                r[0] = E_INTERGENIC, r[1] = 0, r[2] = lf, r[3] = rf, r[6] = refp, r[7] = a0 < 0 ? 0 : ACGT[a0];
            }
            r[10] = a0;
        }
        int32_t *o = rec + i * 12;
#pragma unroll
        for (int q = 0; q < 12; ++q) o[q] = r[q];
    }
}

// ---- the links

// every link end (e < n: pos1[e], else pos2[e - n]) to its slot among the sorted positions; bad = the first end that matches no SNP or several
__global__ __launch_bounds__(256) void k_map_ends(const double *__restrict__ pos1, const double *__restrict__ pos2, int64_t n, const uint32_t *__restrict__ spos,
                                                  int64_t L, int32_t *__restrict__ used, int32_t *__restrict__ slot, unsigned long long *__restrict__ bad) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < 2 * n; e += (int64_t)gridDim.x * 256) {
        const double v = e < n ? pos1[e] : pos2[e - n];
        const int64_t lo = lower_bound_dev<double>(spos, L, v);
        const bool one = lo < L && (double)spos[lo] == v && (lo + 1 == L || (double)spos[lo + 1] != v);
        if (!one) {
            atomicMin(bad, (unsigned long long)e);
            slot[e] = 0;
            continue;
        }
        used[lo] = 1;
        slot[e] = (int32_t)lo;
    }
}

// the annotation row of every link end, and the SNP index of every row (rows = used slots in position order)
__global__ __launch_bounds__(256) void k_map_rows(const int32_t *__restrict__ slot, int64_t n2, const int32_t *__restrict__ used,
                                                  const int32_t *__restrict__ ex, const int32_t *__restrict__ sidx, int64_t L, int32_t *__restrict__ row,
                                                  int32_t *__restrict__ snp_of_row) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n2; e += stride) row[e] = ex[slot[e]];
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < L; s += stride)
        if (used[s]) snp_of_row[ex[s]] = sidx[s];
}

// ascending in the returned key = decreasing in x, NaN last (R's order(decreasing = TRUE), na.last = TRUE); -0 == 0
__global__ __launch_bounds__(256) void k_links_key(const double *__restrict__ x, int64_t n, uint64_t *__restrict__ key, int64_t *__restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        double v = x[i];
        uint64_t k;
        if (v != v) {
            k = ~0ull;
        } else {
            if (v == 0.0) v = 0.0;
            const uint64_t b = (uint64_t)__double_as_longlong(v);
            const uint64_t asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
            k = ~asc;
            if (k == ~0ull) k = ~0ull - 1;   // (no finite value reaches it; kept apart from NaN all the same)
        }
        key[i] = k;
        idx[i] = i;
    }
}

// per sorted link j (source row perm[j]): the two annotation rows, the code pair (3 code1 + code2; codes 0 sy, 1 ns, 2 ig) and whether it is
// a top hit (ARACNE == 1, not syXsy, the two gene regions differ and neither is NA); flag[n] = 0 closes the scan
__global__ __launch_bounds__(256) void k_links_join(const int64_t *__restrict__ perm, int64_t n, const int32_t *__restrict__ row,
                                                    const double *__restrict__ aracne, const int8_t *__restrict__ code, const int32_t *__restrict__ cds,
                                                    int32_t *__restrict__ r1, int32_t *__restrict__ r2, int8_t *__restrict__ pair,
                                                    int64_t *__restrict__ flag) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j <= n; j += (int64_t)gridDim.x * 256) {
        if (j == n) {
            flag[j] = 0;
            continue;
        }
        const int64_t i = perm[j];
        const int32_t a = row[i], b = row[n + i];
        const int32_t pr = code[a] * 3 + code[b];
        const int32_t ca = cds[a], cb = cds[b];
        r1[j] = a;
        r2[j] = b;
        pair[j] = (int8_t)pr;
        flag[j] = (aracne[i] == 1.0 && pr != 0 && ca >= 0 && cb >= 0 && ca != cb) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_links_top(const int64_t *__restrict__ flag, const int64_t *__restrict__ ex, int64_t n, int64_t kmax,
                                                   int64_t *__restrict__ top) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256)
        if (flag[j] && ex[j] < kmax) top[ex[j]] = j;
}

}  // namespace

extern "C" {

int ldw_annot_snps(ldw_ctx *c, const char *ref, int64_t g, const int32_t *seg, int64_t nseg, const int8_t *strand, int64_t nfeat, const int32_t *pos,
                   const uint8_t *alt_mask, int64_t n, int32_t *rec_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(ref && pos && alt_mask && rec_out, LDW_ERR_ARG, "ldw_annot_snps: null argument");
    LDW_REQUIRE(g >= 1 && g < ((int64_t)1 << 31), LDW_ERR_ARG, "ldw_annot_snps: reference length %lld outside 1..2^31-1", (long long)g);
    LDW_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), LDW_ERR_ARG, "ldw_annot_snps: %lld SNPs out of range", (long long)n);
    LDW_REQUIRE(nfeat >= 0 && nseg >= nfeat && nseg < ((int64_t)1 << 28), LDW_ERR_ARG, "ldw_annot_snps: %lld features in %lld segments",
                (long long)nfeat, (long long)nseg);
    LDW_REQUIRE(nseg == 0 || (seg && strand), LDW_ERR_ARG, "ldw_annot_snps: null argument");
    for (int64_t i = 0; i < n; ++i)
        LDW_REQUIRE(pos[i] >= 1 && pos[i] <= g, LDW_ERR_ARG, "ldw_annot_snps: pos[%lld] = %d outside 1..%lld", (long long)i, pos[i], (long long)g);
    // host half: the feature table and the three search orders (features are few: thousands)
    std::vector<int32_t> F((size_t)nfeat * 8, 0), S((size_t)nseg * 4);
    std::vector<int32_t> first((size_t)nfeat, -1);
    int32_t prev = -1;
    for (int64_t s = 0; s < nseg; ++s) {
        const int32_t lo = seg[s * 3], hi = seg[s * 3 + 1], f = seg[s * 3 + 2];
        LDW_REQUIRE(lo >= 1 && lo <= hi && hi <= g, LDW_ERR_ARG, "ldw_annot_snps: segment %lld spans %d..%d, outside 1..%lld", (long long)s, lo, hi,
                    (long long)g);
        LDW_REQUIRE(f == prev || f == prev + 1, LDW_ERR_ARG, "ldw_annot_snps: segment %lld has feature %d after %d (features 0.. in order, contiguous)",
                    (long long)s, f, prev);
        int32_t *Ff = &F[(size_t)f * 8];
        if (f != prev) {
            LDW_REQUIRE(strand[f] == 1 || strand[f] == -1, LDW_ERR_ARG, "ldw_annot_snps: feature %d has strand %d", f, (int)strand[f]);
            Ff[0] = lo, Ff[1] = hi, Ff[2] = strand[f], Ff[3] = (int32_t)s, Ff[4] = 0, Ff[6] = 0;
        }
        Ff[0] = std::min(Ff[0], lo), Ff[1] = std::max(Ff[1], hi);
        S[(size_t)s * 4] = lo, S[(size_t)s * 4 + 1] = hi, S[(size_t)s * 4 + 2] = Ff[6], S[(size_t)s * 4 + 3] = f;
        LDW_REQUIRE((int64_t)Ff[6] + (hi - lo + 1) < ((int64_t)1 << 31), LDW_ERR_ARG, "ldw_annot_snps: feature %d is longer than 2^31", f);
        Ff[4] += 1, Ff[6] += hi - lo + 1;
        prev = f;
    }
    LDW_REQUIRE(prev + 1 == nfeat, LDW_ERR_ARG, "ldw_annot_snps: the segments name %d features, nfeat = %lld", prev + 1, (long long)nfeat);
    std::vector<int32_t> bs((size_t)nfeat), be((size_t)nfeat), st((size_t)nseg);
    std::iota(bs.begin(), bs.end(), 0);
    std::stable_sort(bs.begin(), bs.end(), [&](int32_t a, int32_t b) { return F[(size_t)a * 8] < F[(size_t)b * 8]; });
    for (int64_t r = 0; r < nfeat; ++r) F[(size_t)bs[(size_t)r] * 8 + 5] = (int32_t)r;
    std::iota(be.begin(), be.end(), 0);
    std::stable_sort(be.begin(), be.end(), [&](int32_t a, int32_t b) {
        return F[(size_t)a * 8 + 1] != F[(size_t)b * 8 + 1] ? F[(size_t)a * 8 + 1] < F[(size_t)b * 8 + 1] : F[(size_t)a * 8 + 5] < F[(size_t)b * 8 + 5];
    });
    std::iota(st.begin(), st.end(), 0);
    std::stable_sort(st.begin(), st.end(), [&](int32_t a, int32_t b) { return S[(size_t)a * 4] < S[(size_t)b * 4]; });
    // one int32 image: F S stl stm sti bsl bsf beh bef
    const int64_t nimg = nfeat * 8 + nseg * 4 + 3 * nseg + 4 * nfeat;
    std::vector<int32_t> img((size_t)std::max<int64_t>(nimg, 1));
    int32_t *w = img.data();
    std::copy(F.begin(), F.end(), w);
    std::copy(S.begin(), S.end(), w + nfeat * 8);
    int32_t *stl = w + nfeat * 8 + nseg * 4, *stm = stl + nseg, *sti = stm + nseg, *bsl = sti + nseg, *bsf = bsl + nfeat, *beh = bsf + nfeat,
            *bef = beh + nfeat;
    int32_t run = 0;
    for (int64_t j = 0; j < nseg; ++j) {
        const int32_t s = st[(size_t)j];
        run = std::max(run, S[(size_t)s * 4 + 1]);
        stl[j] = S[(size_t)s * 4], stm[j] = run, sti[j] = s;
    }
    for (int64_t j = 0; j < nfeat; ++j) {
        bsl[j] = F[(size_t)bs[(size_t)j] * 8], bsf[j] = bs[(size_t)j];
        beh[j] = F[(size_t)be[(size_t)j] * 8 + 1], bef[j] = be[(size_t)j];
    }
    Carve cv;
    auto d_img = cv.take<int32_t>(nimg);
    auto d_ref = cv.take<char>(g);
    auto d_pos = cv.take<int32_t>(n);
    auto d_alt = cv.take<uint8_t>(n);
    auto d_rec = cv.take<int32_t>(n * LDW_ANNOT_REC);
    if (int rc = cv.reserve(c->annot_work)) return rc;
    LDW_HIP(hipMemcpyAsync(d_img, img.data(), (size_t)nimg * 4, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(d_ref, ref, (size_t)g, hipMemcpyHostToDevice, c->stream));
    if (n > 0) {
        LDW_HIP(hipMemcpyAsync(d_pos, pos, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemcpyAsync(d_alt, alt_mask, (size_t)n, hipMemcpyHostToDevice, c->stream));
        const int32_t *di = d_img;
        Tables t{di, di + nfeat * 8, di + (stl - w), di + (stm - w), di + (sti - w), di + (bsl - w), di + (bsf - w), di + (beh - w), di + (bef - w), nfeat, nseg};
        LDW_LAUNCH(k_annot_snp, grid_of(n), dim3(256), 0, c->stream, t, d_ref, g, d_pos, d_alt, n, d_rec);
        LDW_HIP(hipMemcpyAsync(rec_out, d_rec, (size_t)n * LDW_ANNOT_REC * 4, hipMemcpyDeviceToHost, c->stream));
    }
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

int ldw_annot_map(ldw_ctx *c, const double *pos1, const double *pos2, int64_t n, const int32_t *POS, int64_t L, int32_t *snp_out, int64_t *rows_out,
                  int64_t *bad_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(POS && snp_out && rows_out && bad_out && (n == 0 || (pos1 && pos2)), LDW_ERR_ARG, "ldw_annot_map: null argument");
    LDW_REQUIRE(n >= 0 && n < ((int64_t)1 << 40), LDW_ERR_ARG, "ldw_annot_map: %lld links out of range", (long long)n);
    LDW_REQUIRE(L >= 1 && L < ((int64_t)1 << 31), LDW_ERR_ARG, "ldw_annot_map: L = %lld out of range", (long long)L);
    for (int64_t i = 0; i < L; ++i) LDW_REQUIRE(POS[i] >= 1, LDW_ERR_ARG, "ldw_annot_map: POS[%lld] = %d is not positive", (long long)i, POS[i]);
    c->annot_n = -1;
    size_t sort_bytes = 0, scan_bytes = 0;
    LDW_HIP((prim_sort_pairs_bytes<uint32_t, int32_t>((size_t)L, 0, 32, c->stream, &sort_bytes)));
    LDW_HIP(prim_scan_bytes<int32_t>((size_t)L + 1, c->stream, &scan_bytes));
    Carve cv;
    auto d_pos = cv.take<uint32_t>(L), spos = cv.take<uint32_t>(L);
    auto iota = cv.take<int32_t>(L), sidx = cv.take<int32_t>(L);
    auto p1 = cv.take<double>(n), p2 = cv.take<double>(n);
    auto used = cv.take<int32_t>(L + 1), ex = cv.take<int32_t>(L + 1), slot = cv.take<int32_t>(2 * n), snp = cv.take<int32_t>(L);
    auto bad = cv.take<unsigned long long>(1);
    auto tmp = cv.take<char>((int64_t)std::max(sort_bytes, scan_bytes));
    if (int rc = cv.reserve(c->annot_work)) return rc;
    if (int rc = c->annot_keep.reserve((size_t)std::max<int64_t>(2 * n, 1) * 4)) return rc;
    if (n > 0) {
        LDW_HIP(hipMemcpyAsync(p1, pos1, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemcpyAsync(p2, pos2, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    }
    LDW_HIP(hipMemsetAsync(used, 0, (size_t)(L + 1) * 4, c->stream));
    LDW_HIP(hipMemsetAsync(bad, 0xff, 8, c->stream));
    if (int rc = sort_positions(c, POS, L, 32, d_pos, iota, spos, sidx, tmp, sort_bytes)) return rc;
    if (n > 0) {
        LDW_LAUNCH(k_map_ends, grid_of(2 * n), dim3(256), 0, c->stream, p1, p2, n, spos, L, used, slot, bad);
    }
    LDW_HIP((prim_exclusive_sum<int32_t>(tmp, scan_bytes, used, ex, (size_t)L + 1, c->stream)));
    LDW_LAUNCH(k_map_rows, grid_of(std::max<int64_t>(2 * n, L)), dim3(256), 0, c->stream, slot, 2 * n, used, ex, sidx, L,
                       c->annot_keep.as<int32_t>(), snp);
    unsigned long long h_bad = 0;
    int32_t h_rows = 0;
    LDW_HIP(hipMemcpyAsync(&h_bad, bad, 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(&h_rows, ex + L, 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    *bad_out = h_bad == ~0ull ? -1 : (int64_t)h_bad;
    *rows_out = h_rows;
    if (h_rows > 0) {
        LDW_HIP(hipMemcpyAsync(snp_out, snp, (size_t)h_rows * 4, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
    }
    if (*bad_out < 0) {
        c->annot_n = n;
        c->annot_rows = h_rows;
    }
    return LDW_OK;
}

int ldw_annot_links(ldw_ctx *c, const double *key, const double *aracne, int64_t n, const int8_t *code, const int32_t *cds_id, int64_t rows,
                    int64_t max_tophits, int64_t *perm_out, int32_t *r1_out, int32_t *r2_out, int8_t *pair_out, int64_t *top_out, int64_t *n_top_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(c->annot_n >= 0, LDW_ERR_STATE, "ldw_annot_links: call ldw_annot_map first");
    LDW_REQUIRE(n == c->annot_n && rows == c->annot_rows, LDW_ERR_ARG, "ldw_annot_links: %lld links / %lld rows, ldw_annot_map had %lld / %lld",
                (long long)n, (long long)rows, (long long)c->annot_n, (long long)c->annot_rows);
    LDW_REQUIRE(max_tophits >= 0 && n_top_out && (n == 0 || (key && aracne && code && cds_id && perm_out && r1_out && r2_out && pair_out)) &&
                    (max_tophits == 0 || n == 0 || top_out),
                LDW_ERR_ARG, "ldw_annot_links: null or negative argument");
    for (int64_t r = 0; r < rows; ++r) LDW_REQUIRE(code[r] >= 0 && code[r] <= 2, LDW_ERR_ARG, "ldw_annot_links: code[%lld] = %d", (long long)r, (int)code[r]);
    *n_top_out = 0;
    if (n == 0) return LDW_OK;
    size_t sort_bytes = 0, scan_bytes = 0;
    LDW_HIP((prim_sort_pairs_bytes<uint64_t, int64_t>((size_t)n, 0, 64, c->stream, &sort_bytes)));
    LDW_HIP(prim_scan_bytes<int64_t>((size_t)n + 1, c->stream, &scan_bytes));
    const int64_t kmax = std::min(max_tophits, n);
    Carve cv;
    auto d_key = cv.take<double>(n), d_ar = cv.take<double>(n);
    auto d_code = cv.take<int8_t>(rows);
    auto d_cds = cv.take<int32_t>(rows);
    auto k1 = cv.take<uint64_t>(n), k2 = cv.take<uint64_t>(n);
    auto iv = cv.take<int64_t>(n), perm = cv.take<int64_t>(n);
    auto r1 = cv.take<int32_t>(n), r2 = cv.take<int32_t>(n);
    auto pair = cv.take<int8_t>(n);
    auto flag = cv.take<int64_t>(n + 1), ex = cv.take<int64_t>(n + 1), top = cv.take<int64_t>(kmax);
    auto tmp = cv.take<char>((int64_t)std::max(sort_bytes, scan_bytes));
    if (int rc = cv.reserve(c->annot_work)) return rc;
    LDW_HIP(hipMemcpyAsync(d_key, key, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(d_ar, aracne, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    if (rows > 0) {
        LDW_HIP(hipMemcpyAsync(d_code, code, (size_t)rows, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemcpyAsync(d_cds, cds_id, (size_t)rows * 4, hipMemcpyHostToDevice, c->stream));
    }
    LDW_LAUNCH(k_links_key, grid_of(n), dim3(256), 0, c->stream, d_key, n, k1, iv);
    LDW_HIP((prim_sort_pairs<uint64_t, int64_t>(tmp, sort_bytes, k1, k2, iv, perm, (size_t)n, 0, 64, c->stream)));
    LDW_LAUNCH(k_links_join, grid_of(n + 1), dim3(256), 0, c->stream, perm, n, c->annot_keep.as<int32_t>(), d_ar, d_code, d_cds, r1, r2, pair, flag);
    LDW_HIP((prim_exclusive_sum<int64_t>(tmp, scan_bytes, flag, ex, (size_t)n + 1, c->stream)));
    if (kmax > 0) {
        LDW_LAUNCH(k_links_top, grid_of(n), dim3(256), 0, c->stream, flag, ex, n, kmax, top);
    }
    int64_t total = 0;
    LDW_HIP(hipMemcpyAsync(&total, ex + n, 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(perm_out, perm, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(r1_out, r1, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(r2_out, r2, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(pair_out, pair, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    const int64_t nt = std::min(total, kmax);
    if (nt > 0) {
        LDW_HIP(hipMemcpyAsync(top_out, top, (size_t)nt * 8, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
    }
    *n_top_out = nt;
    return LDW_OK;
}

}  // extern "C"

// The host-only parts of the sequence-level analyses (ldw_nj.hip, ldw_pars.hip, ldw_lineage.hip, ldw_perm.hip): the rules their entry
// points share (a list of SNP indices, a list of cluster labels, the distinct SNPs of a list of pairs, a budget with its test hook) and the host plans
// of ldw_links_stratified and ldw_links_permuted.  A check returns the offender; the message and LDW_REQUIRE stay at the call site (as ldw_pass_plan.h).
// Plain C++, no HIP: tests/host/seq_plan_check.cpp reads this header with g++ (tests/test_seq_plan_host.py), also under the address and UB sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace ldw {

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline int64_t round_up(int64_t x, int64_t m) { return ceil_div(x, m) * m; }

// the integer of an environment variable, -1 where it is not set (atoll: text that is no number reads as 0); read at every call
inline long long env_int(const char *name) { const char *e = getenv(name); return e ? atoll(e) : -1; }
// what the budget gives, unless the test hook `hook` (LDW_PARS_CHUNK, LDW_LIN_CHUNK, LDW_PERM_BATCH, LDW_PERM_CHUNK, LDW_NJ_BATCH) holds an integer >= 1
inline int64_t budget_or_env(int64_t value, const char *hook) { const long long k = env_int(hook); return k >= 1 ? (int64_t)k : value; }

// the first k with idx[k] outside 0..L-1, or -1
inline int64_t first_bad_index(const int32_t *idx, int64_t n, int64_t L) {
    for (int64_t k = 0; k < n; ++k)
        if (idx[k] < 0 || idx[k] >= L) return k;
    return -1;
}
// the same for K pairs taken pair by pair, a before b: the list that holds the first offender, at *k; null where there is none
inline const int32_t *first_bad_pair(const int32_t *a, const int32_t *b, int64_t K, int64_t L, int64_t *k) {
    const int64_t ia = first_bad_index(a, K, L), ib = first_bad_index(b, K, L);
    const bool in_a = ia >= 0 && (ib < 0 || ia <= ib);
    *k = in_a ? ia : ib;
    return in_a ? a : ib >= 0 ? b : nullptr;
}

// labels[N]: -1 (the sequence is left out) or a cluster 0..C-1
struct LabelSet {
    int64_t bad = -1;   // the first sequence whose label is neither, or -1
    int64_t P = 0;      // labelled sequences (of all N where bad < 0)
    static LabelSet scan(const int32_t *labels, int64_t N, int32_t C) {
        LabelSet r;
        for (int64_t s = 0; s < N && r.bad < 0; ++s)
            if (labels[s] < -1 || labels[s] >= C) r.bad = s;
            else r.P += labels[s] >= 0;
        return r;
    }
    // out[k] = the weight of cluster k, out[C] = of all labelled sequences: each a long double sum in sequence order, rounded once.  THE one summation:
    // ldw_links_permuted's mi_obs equals ldw_links_stratified's mi_all bit for bit (tests/test_perm_gpu.py) because both take out[C] from here.
    static void neff(const int32_t *labels, const double *hdw, int64_t N, int32_t C, double *out) {
        std::vector<long double> sums((size_t)C + 1, 0.0L);
        for (int64_t s = 0; s < N; ++s)
            if (labels[s] >= 0) sums[(size_t)labels[s]] += (long double)hdw[s], sums[(size_t)C] += (long double)hdw[s];
        for (size_t k = 0; k <= (size_t)C; ++k) out[k] = (double)sums[k];
    }
};

// the distinct SNPs of one or two lists (b may be null) in ascending order, and the place of a listed SNP among them
struct DistinctSlots {
    std::vector<int32_t> d;
    DistinctSlots() = default;
    DistinctSlots(const int32_t *a, int64_t na, const int32_t *b, int64_t nb) { assign(a, na, b, nb); }
    void assign(const int32_t *a, int64_t na, const int32_t *b, int64_t nb) {
        d.assign(a, a + na);
        if (b) d.insert(d.end(), b, b + nb);
        std::sort(d.begin(), d.end());
        d.erase(std::unique(d.begin(), d.end()), d.end());
    }
    int32_t slot(int32_t snp) const { return (int32_t)(std::lower_bound(d.begin(), d.end(), snp) - d.begin()); }
};

// ldw_links_stratified.  The labelled sequences ordered by (label, V, sequence): position p of that order is bit p & 63 of word p >> 6.
// A piece is a maximal run of positions of ONE word that share label and V; a cluster is the range clu_piece[k] .. clu_piece[k + 1] of pieces.  A job of
// k_lin_pairs is one large cluster (job_count 0, job_first the cluster) or up to 64 small ones (job_count of them from small[job_first]); a cluster
// without a member is in neither.
constexpr int LIN_SMALL = 16;   // a cluster of at most this many pieces is walked by one lane

struct LinPlan {
    std::vector<int32_t> perm, pc_word, job_first, job_count, small;   // perm[P]: the sequence at a position; per piece its word,
    std::vector<uint64_t> pc_mask;                                     // its bits of that word
    std::vector<int64_t> pc_v, clu_piece;                              // and the V its sequences share; clu_piece[C + 1]
};

// labels as LabelSet::scan accepted them with P labelled sequences; V[N] the sequences' fixed-point weights
inline LinPlan build_lin_plan(const int32_t *labels, const int64_t *V, int64_t N, int32_t C, int64_t P) {
    LinPlan pl;
    pl.perm.reserve((size_t)P);
    for (int64_t s = 0; s < N; ++s)
        if (labels[s] >= 0) pl.perm.push_back((int32_t)s);
    std::sort(pl.perm.begin(), pl.perm.end(), [&](int32_t x, int32_t y) {
        if (labels[x] != labels[y]) return labels[x] < labels[y];
        if (V[x] != V[y]) return V[x] < V[y];
        return x < y;
    });
    pl.clu_piece.assign((size_t)C + 1, 0);
    for (int64_t p = 0; p < P;) {
        const int32_t s = pl.perm[(size_t)p];
        int64_t q = p + 1;
        while (q < P && (q >> 6) == (p >> 6) && labels[pl.perm[(size_t)q]] == labels[s] && V[pl.perm[(size_t)q]] == V[s]) ++q;
        const int n = (int)(q - p);
        pl.pc_word.push_back((int32_t)(p >> 6));
        pl.pc_mask.push_back((n == 64 ? ~0ull : ((1ull << n) - 1ull)) << (p & 63));
        pl.pc_v.push_back(V[s]);
        ++pl.clu_piece[(size_t)labels[s] + 1];
        p = q;
    }
    for (int32_t k = 0; k < C; ++k) pl.clu_piece[(size_t)k + 1] += pl.clu_piece[(size_t)k];
    for (int32_t k = 0; k < C; ++k) {
        const int64_t n = pl.clu_piece[(size_t)k + 1] - pl.clu_piece[(size_t)k];
        if (n > LIN_SMALL) pl.job_first.push_back(k), pl.job_count.push_back(0);
        else if (n > 0) pl.small.push_back(k);
    }
    for (size_t s0 = 0; s0 < pl.small.size(); s0 += 64)
        pl.job_first.push_back((int32_t)s0), pl.job_count.push_back((int32_t)std::min<size_t>(64, pl.small.size() - s0));
    return pl;
}

// ldw_links_permuted: the labelled sequences by (label, sequence), a counting sort, and their V in that order
struct PermOrder {
    std::vector<int32_t> order0;
    std::vector<int64_t> v0;
};
inline PermOrder perm_order0(const int32_t *labels, const int64_t *V, int64_t N, int32_t C) {
    std::vector<int64_t> first((size_t)C + 1, 0);
    for (int64_t s = 0; s < N; ++s)
        if (labels[s] >= 0) ++first[(size_t)labels[s] + 1];
    for (int32_t k = 0; k < C; ++k) first[(size_t)k + 1] += first[(size_t)k];
    PermOrder o;
    o.order0.resize((size_t)first[(size_t)C]);
    o.v0.resize((size_t)first[(size_t)C]);
    for (int64_t s = 0; s < N; ++s)
        if (labels[s] >= 0) {
            const int64_t p = first[(size_t)labels[s]]++;
            o.order0[(size_t)p] = (int32_t)s;
            o.v0[(size_t)p] = V[s];
        }
    return o;
}

}  // namespace ldw

// Host check of the host-only parts of the sequence-level analyses — the SAME source the library compiles (ldweaver_amd/csrc/ldw_seq_plan.h): the index
// and label rules, the one neff summation, the distinct SNPs of a list, the budget hook, and the host plans of ldw_links_stratified (against brute
// force) and ldw_links_permuted.  Prints one line per group; exit code 0 iff nothing failed.
//   (tests/test_seq_plan_host.py builds it with g++ -O1 -std=c++17 and runs it; it is also the program to run under -fsanitize=address,undefined)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../ldweaver_amd/csrc/ldw_seq_plan.h"

using namespace ldw;

static int checks = 0, failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        ++checks;                                 \
        if (!(cond)) {                            \
            ++failures;                           \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                  \
            printf("\n");                         \
        }                                         \
    } while (0)

static void check_indices() {
    CHECK(first_bad_index(nullptr, 0, 10) == -1, "empty list");
    const std::vector<int32_t> ok = {0, 9, 5, 0, 9};
    CHECK(first_bad_index(ok.data(), 5, 10) == -1, "0 and L - 1 are inside");
    CHECK(first_bad_index(ok.data(), 5, 9) == 1, "L itself is outside: got %lld", (long long)first_bad_index(ok.data(), 5, 9));
    std::vector<int32_t> v = ok;
    v[0] = -1;
    CHECK(first_bad_index(v.data(), 5, 10) == 0, "first offender");
    v = ok, v[4] = 10;
    CHECK(first_bad_index(v.data(), 5, 10) == 4, "last offender");
    v[2] = -7;
    CHECK(first_bad_index(v.data(), 5, 10) == 2, "the first of two");
    CHECK(first_bad_index(ok.data(), 5, 0) == 0, "no SNPs at all");
    // pairs: pair by pair, a before b
    int64_t k = 99;
    CHECK(first_bad_pair(nullptr, nullptr, 0, 10, &k) == nullptr && k == -1, "no pairs");
    const std::vector<int32_t> a = {1, 2, 3, 4}, b = {5, 6, 7, 8};
    CHECK(first_bad_pair(a.data(), b.data(), 4, 10, &k) == nullptr && k == -1, "all inside");
    std::vector<int32_t> a2 = a, b2 = b;
    a2[3] = 10, b2[1] = -1;
    CHECK(first_bad_pair(a2.data(), b2.data(), 4, 10, &k) == b2.data() && k == 1, "b's pair comes first: k %lld", (long long)k);
    a2[1] = 11;
    CHECK(first_bad_pair(a2.data(), b2.data(), 4, 10, &k) == a2.data() && k == 1, "the same pair: a before b");
    CHECK(first_bad_pair(a2.data(), b.data(), 4, 10, &k) == a2.data() && k == 1, "a alone");
    CHECK(first_bad_pair(a.data(), b2.data(), 4, 10, &k) == b2.data() && k == 1, "b alone");
    printf("indices: done\n");
}

static void check_labels() {
    LabelSet r = LabelSet::scan(nullptr, 0, 3);
    CHECK(r.bad == -1 && r.P == 0, "empty list");
    const std::vector<int32_t> ok = {-1, 0, 2, -1, 1, 2};
    r = LabelSet::scan(ok.data(), 6, 3);
    CHECK(r.bad == -1 && r.P == 4, "-1 and C - 1 are labels: bad %lld P %lld", (long long)r.bad, (long long)r.P);
    r = LabelSet::scan(ok.data(), 6, 2);
    CHECK(r.bad == 2, "C itself is none: bad %lld", (long long)r.bad);
    std::vector<int32_t> v = ok;
    v[0] = -2;
    CHECK(LabelSet::scan(v.data(), 6, 3).bad == 0, "first offender");
    v = ok, v[5] = 3;
    CHECK(LabelSet::scan(v.data(), 6, 3).bad == 5, "last offender");
    v[3] = -2;
    CHECK(LabelSet::scan(v.data(), 6, 3).bad == 3, "the first of two");
    const std::vector<int32_t> none(50, -1);
    r = LabelSet::scan(none.data(), 50, 4);
    CHECK(r.bad == -1 && r.P == 0, "every label -1: P %lld", (long long)r.P);
    printf("labels: done\n");
}

// weights whose sums depend on the order and on the precision they are added in
static void check_neff() {
    for (int C : {1, 3, 7}) {
        const int64_t N = 200;
        std::vector<int32_t> labels((size_t)N);
        std::vector<double> hdw((size_t)N);
        for (int64_t s = 0; s < N; ++s) {
            labels[(size_t)s] = s % 5 == 4 ? -1 : (int32_t)((s * 7 + s / 3) % C);
            hdw[(size_t)s] = s % 2 ? 1.0 : (s % 4 ? 1e16 : -1e16 + 3.0);
            if (s % 11 == 0) hdw[(size_t)s] = 1.0 / (double)(s + 3);
        }
        std::vector<double> got((size_t)C + 1, -1.0);
        LabelSet::neff(labels.data(), hdw.data(), N, C, got.data());
        long double all = 0.0L, rev = 0.0L;
        double all_d = 0.0;
        for (int64_t s = 0; s < N; ++s)
            if (labels[(size_t)s] >= 0) all += (long double)hdw[(size_t)s], all_d += hdw[(size_t)s];
        for (int64_t s = N - 1; s >= 0; --s)
            if (labels[(size_t)s] >= 0) rev += (long double)hdw[(size_t)s];
        CHECK(got[(size_t)C] == (double)all, "C %d: total %.17g, in sequence order %.17g", C, got[(size_t)C], (double)all);
        CHECK((double)rev != (double)all || all_d != (double)all, "C %d: the weights do not tell one order or precision from another", C);
        for (int k = 0; k < C; ++k) {
            long double one = 0.0L;
            for (int64_t s = 0; s < N; ++s)
                if (labels[(size_t)s] == k) one += (long double)hdw[(size_t)s];
            CHECK(got[(size_t)k] == (double)one, "C %d cluster %d: %.17g, in sequence order %.17g", C, k, got[(size_t)k], (double)one);
        }
    }
    // a cluster without a member, and no labelled sequence at all
    const std::vector<int32_t> labels = {2, -1, 0, 2};
    const std::vector<double> hdw = {0.5, 100.0, 0.25, 0.125};
    double out[4];
    LabelSet::neff(labels.data(), hdw.data(), 4, 3, out);
    CHECK(out[0] == 0.25 && out[1] == 0.0 && out[2] == 0.625 && out[3] == 0.875, "small case: %g %g %g %g", out[0], out[1], out[2], out[3]);
    const std::vector<int32_t> none(4, -1);
    LabelSet::neff(none.data(), hdw.data(), 4, 3, out);
    CHECK(out[0] == 0 && out[1] == 0 && out[2] == 0 && out[3] == 0, "no labelled sequence");
    printf("neff: done\n");
}

static bool ascending_distinct(const std::vector<int32_t> &d) {
    for (size_t i = 1; i < d.size(); ++i)
        if (d[i - 1] >= d[i]) return false;
    return true;
}
static void check_distinct() {
    const std::vector<int32_t> a = {9, 3, 3, 7, 0, 9}, b = {4, 3, 11, 0, 0, 2};
    {
        const DistinctSlots ds(a.data(), 6, b.data(), 6);
        CHECK(ds.d == std::vector<int32_t>({0, 2, 3, 4, 7, 9, 11}), "two lists: %zu distinct", ds.d.size());
        for (int32_t x : a) CHECK(ds.d[(size_t)ds.slot(x)] == x, "a: slot of %d", x);
        for (int32_t x : b) CHECK(ds.d[(size_t)ds.slot(x)] == x, "b: slot of %d", x);
    }
    {
        const DistinctSlots ds(a.data(), 6, a.data(), 6);   // a == b
        CHECK(ds.d == std::vector<int32_t>({0, 3, 7, 9}), "a == b: %zu distinct", ds.d.size());
        for (int32_t x : a) CHECK(ds.d[(size_t)ds.slot(x)] == x, "a == b: slot of %d", x);
    }
    {
        const DistinctSlots ds(a.data(), 6, nullptr, 0);   // one list
        CHECK(ds.d == std::vector<int32_t>({0, 3, 7, 9}), "b null: %zu distinct", ds.d.size());
        for (int32_t x : a) CHECK(ds.d[(size_t)ds.slot(x)] == x, "b null: slot of %d", x);
    }
    {
        const std::vector<int32_t> same(1000, 123456);
        const DistinctSlots ds(same.data(), 1000, same.data(), 1000);
        CHECK(ds.d.size() == 1 && ds.d[0] == 123456 && ds.slot(123456) == 0, "one SNP 1000 times: %zu distinct", ds.d.size());
    }
    {
        DistinctSlots ds(a.data(), 6, b.data(), 6);   // assigned again: nothing of the first list stays
        ds.assign(b.data() + 2, 2, a.data() + 3, 1);
        CHECK(ds.d == std::vector<int32_t>({0, 7, 11}), "assign: %zu distinct", ds.d.size());
        CHECK(ds.slot(0) == 0 && ds.slot(7) == 1 && ds.slot(11) == 2, "assign: slots");
    }
    {
        uint32_t x = 12345u;
        std::vector<int32_t> p(300), q(300);
        for (size_t i = 0; i < 300; ++i) {
            x = x * 1664525u + 1013904223u, p[i] = (int32_t)((x >> 8) % 97u);
            x = x * 1664525u + 1013904223u, q[i] = (int32_t)((x >> 8) % 5000u);
        }
        const DistinctSlots ds(p.data(), 300, q.data(), 300);
        bool back = ascending_distinct(ds.d);
        for (size_t i = 0; i < 300; ++i) back = back && ds.d[(size_t)ds.slot(p[i])] == p[i] && ds.d[(size_t)ds.slot(q[i])] == q[i];
        CHECK(back, "random lists: ascending, distinct, and every input found");
    }
    printf("distinct: done\n");
}

static void check_budget() {
    const char *hook = "LDW_SEQ_PLAN_CHECK_HOOK";
    unsetenv(hook);
    CHECK(env_int(hook) == -1 && budget_or_env(40, hook) == 40, "unset");
    setenv(hook, "0", 1);
    CHECK(budget_or_env(40, hook) == 40, "0 keeps the budget");
    setenv(hook, "-3", 1);
    CHECK(budget_or_env(40, hook) == 40, "-3 keeps the budget");
    setenv(hook, "7", 1);
    CHECK(budget_or_env(40, hook) == 7 && env_int(hook) == 7, "7 forces 7");
    setenv(hook, "1", 1);
    CHECK(budget_or_env(40, hook) == 1, "1 forces 1");
    setenv(hook, "5000000000", 1);
    CHECK(budget_or_env(40, hook) == 5000000000ll, "past 32 bits");
    setenv(hook, "seven", 1);
    CHECK(budget_or_env(40, hook) == 40 && env_int(hook) == 0, "text that is no number reads as 0");
    setenv(hook, "", 1);
    CHECK(budget_or_env(40, hook) == 40, "empty");
    setenv(hook, "7", 1);
    unsetenv(hook);
    CHECK(budget_or_env(40, hook) == 40, "read at every call");
    CHECK(ceil_div(0, 64) == 0 && ceil_div(1, 64) == 1 && ceil_div(64, 64) == 1 && ceil_div(65, 64) == 2, "ceil_div");
    CHECK(round_up(0, 256) == 0 && round_up(1, 256) == 256 && round_up(256, 256) == 256 && round_up(257, 256) == 512, "round_up");
    printf("budget: done\n");
}

// labelling 0: all in cluster 0 (the others empty); 1: round-robin; 2: round-robin over all clusters but cluster 1 (empty; with C = 1 as 0).
// V 0: all equal; 1: all distinct; 2: two values alternating.  An unlabelled sequence stands in front of every other labelled one.
static void one_lin_plan(int64_t P, int32_t C, int lab, int vmode) {
    std::vector<int32_t> labels;
    std::vector<int64_t> V;
    for (int64_t m = 0; m < P; ++m) {
        if (m % 2 == 0) labels.push_back(-1), V.push_back(5);
        int32_t l = 0;
        if (lab == 1) l = (int32_t)(m % C);
        if (lab == 2 && C > 1) l = (int32_t)(m % (C - 1)), l += l >= 1;
        labels.push_back(l);
        V.push_back(vmode == 0 ? 1000 : vmode == 1 ? 7 * P - 3 * m : (m % 2 ? 11 : 1000));
    }
    const int64_t N = (int64_t)labels.size();
    CHECK(LabelSet::scan(labels.data(), N, C).P == P, "the case has P labelled sequences");
    const LinPlan pl = build_lin_plan(labels.data(), V.data(), N, C, P);
    const char *fmt = "P %lld C %d labels %d V %d: %s";
#define PLAN_CHECK(cond, what) CHECK(cond, fmt, (long long)P, (int)C, lab, vmode, what)
    // the order: every labelled sequence once, ascending in (label, V, sequence)
    bool order_ok = (int64_t)pl.perm.size() == P;
    std::vector<int> seen_seq((size_t)N, 0);
    for (int64_t p = 0; order_ok && p < P; ++p) {
        const int32_t s = pl.perm[(size_t)p];
        order_ok = s >= 0 && s < N && labels[(size_t)s] >= 0 && !seen_seq[(size_t)s]++;
        if (order_ok && p > 0) {
            const int32_t r = pl.perm[(size_t)p - 1];
            const bool less = labels[(size_t)r] != labels[(size_t)s] ? labels[(size_t)r] < labels[(size_t)s] : V[(size_t)r] != V[(size_t)s] ? V[(size_t)r] < V[(size_t)s] : r < s;
            order_ok = less;
        }
    }
    PLAN_CHECK(order_ok, "perm is the labelled sequences by (label, V, sequence)");
    if (!order_ok) return;
    // the pieces: every position once, within one word, uniform in (label, V), maximal, in the order of the positions
    const size_t n_pc = pl.pc_word.size();
    PLAN_CHECK(pl.pc_mask.size() == n_pc && pl.pc_v.size() == n_pc && (int64_t)pl.clu_piece.size() == (int64_t)C + 1, "sizes");
    std::vector<int> cover((size_t)P, 0);
    std::vector<int32_t> piece_label(n_pc, -1);
    bool in_word = true, uniform = true, ordered = true, maximal = true;
    int64_t prev_last = -1;
    for (size_t q = 0; q < n_pc; ++q) {
        const int64_t w = pl.pc_word[q];
        const uint64_t m = pl.pc_mask[q];
        in_word = in_word && m != 0 && w >= 0 && w * 64 < P;
        int64_t first = -1, last = -1;
        for (int bit = 0; bit < 64; ++bit)
            if ((m >> bit) & 1ull) {
                const int64_t p = w * 64 + bit;
                if (p >= P) {
                    in_word = false;
                    continue;
                }
                ++cover[(size_t)p];
                const int32_t s = pl.perm[(size_t)p];
                if (first < 0) first = p, piece_label[q] = labels[(size_t)s];
                uniform = uniform && labels[(size_t)s] == piece_label[q] && V[(size_t)s] == pl.pc_v[q] && (last < 0 || p == last + 1);
                last = p;
            }
        ordered = ordered && first == prev_last + 1;
        if (q > 0 && first > 0 && (first & 63) != 0) {   // the piece in front, in the same word, differs in label or V
            const int32_t s = pl.perm[(size_t)first], r = pl.perm[(size_t)first - 1];
            maximal = maximal && (labels[(size_t)r] != labels[(size_t)s] || V[(size_t)r] != V[(size_t)s]);
        }
        prev_last = last;
    }
    bool once = true;
    for (int64_t p = 0; p < P; ++p) once = once && cover[(size_t)p] == 1;
    PLAN_CHECK(once, "the pieces hold every position exactly once");
    PLAN_CHECK(in_word, "no piece is empty, leaves its word or the positions");
    PLAN_CHECK(uniform, "every piece is a run of one label and one V");
    PLAN_CHECK(ordered && prev_last == P - 1, "the pieces follow the positions");
    PLAN_CHECK(maximal, "pieces of one word that could be one are one");
    // the clusters' ranges against the labels
    bool ranges = pl.clu_piece[0] == 0 && pl.clu_piece[(size_t)C] == (int64_t)n_pc;
    for (int32_t k = 0; ranges && k < C; ++k) {
        ranges = pl.clu_piece[(size_t)k] <= pl.clu_piece[(size_t)k + 1];
        for (int64_t q = pl.clu_piece[(size_t)k]; ranges && q < pl.clu_piece[(size_t)k + 1]; ++q) ranges = piece_label[(size_t)q] == k;
    }
    PLAN_CHECK(ranges, "clu_piece cuts the pieces by label");
    if (!ranges) return;
    // the jobs
    std::vector<int64_t> members((size_t)C, 0);
    for (int64_t s = 0; s < N; ++s)
        if (labels[(size_t)s] >= 0) ++members[(size_t)labels[(size_t)s]];
    std::vector<int> in_job((size_t)C, 0);
    std::vector<int> small_used(pl.small.size(), 0);
    bool jobs = pl.job_first.size() == pl.job_count.size(), large_rule = true, sixty_four = true;
    size_t next_small = 0, n_small_jobs = 0;
    for (size_t j = 0; jobs && j < pl.job_first.size(); ++j) {
        const int32_t first = pl.job_first[j], count = pl.job_count[j];
        if (count == 0) {
            jobs = first >= 0 && first < C;
            if (jobs) ++in_job[(size_t)first], large_rule = large_rule && pl.clu_piece[(size_t)first + 1] - pl.clu_piece[(size_t)first] > LIN_SMALL;
            large_rule = large_rule && n_small_jobs == 0;   // the large jobs come first
        } else {
            jobs = count >= 1 && count <= 64 && first >= 0 && (size_t)first == next_small && (size_t)first + (size_t)count <= pl.small.size();
            for (int32_t l = 0; jobs && l < count; ++l) {
                const int32_t k = pl.small[(size_t)first + (size_t)l];
                jobs = k >= 0 && k < C;
                if (jobs) {
                    ++in_job[(size_t)k], ++small_used[(size_t)first + (size_t)l];
                    const int64_t n = pl.clu_piece[(size_t)k + 1] - pl.clu_piece[(size_t)k];
                    large_rule = large_rule && n >= 1 && n <= LIN_SMALL;
                }
            }
            next_small += (size_t)count, ++n_small_jobs;
            sixty_four = sixty_four && (count == 64 || (size_t)first + (size_t)count == pl.small.size());   // only the last one is short
        }
    }
    PLAN_CHECK(jobs && next_small == pl.small.size(), "the jobs are well formed and take every small cluster");
    PLAN_CHECK(large_rule, "a cluster is a job of its own iff it has more than LIN_SMALL pieces");
    PLAN_CHECK(sixty_four && n_small_jobs == (pl.small.size() + 63) / 64, "the small clusters go 64 to a job");
    bool each_once = true;
    for (int32_t k = 0; k < C; ++k) each_once = each_once && in_job[(size_t)k] == (members[(size_t)k] > 0 ? 1 : 0);
    PLAN_CHECK(each_once, "a cluster with members is in one job, one without in none");
    for (size_t i = 1; i < pl.small.size(); ++i) each_once = each_once && pl.small[i - 1] < pl.small[i];
    PLAN_CHECK(each_once, "the small clusters are listed in ascending order");
#undef PLAN_CHECK
}

static void check_lin_plan() {
    for (int64_t P : {1, 63, 64, 65, 128, 129})
        for (int32_t C : {1, 3, 70})
            for (int lab = 0; lab < 3; ++lab)
                for (int vmode = 0; vmode < 3; ++vmode) one_lin_plan(P, C, lab, vmode);
    {   // 70 clusters, every one small: the job of 64 and the job of 6
        std::vector<int32_t> labels(129);
        std::vector<int64_t> V(129, 3);
        for (size_t s = 0; s < 129; ++s) labels[s] = (int32_t)(s % 70);
        const LinPlan pl = build_lin_plan(labels.data(), V.data(), 129, 70, 129);
        CHECK(pl.small.size() == 70 && pl.job_first == std::vector<int32_t>({0, 64}) && pl.job_count == std::vector<int32_t>({64, 6}),
              "70 small clusters: %zu jobs", pl.job_first.size());
    }
    {   // the threshold itself: LIN_SMALL pieces are small, one more is a job of its own
        for (int n : {LIN_SMALL, LIN_SMALL + 1}) {
            std::vector<int32_t> labels((size_t)n, 0);
            std::vector<int64_t> V((size_t)n);
            for (int s = 0; s < n; ++s) V[(size_t)s] = s;   // all distinct: a piece per sequence
            const LinPlan pl = build_lin_plan(labels.data(), V.data(), n, 1, n);
            CHECK(pl.pc_word.size() == (size_t)n && pl.job_first.size() == 1 && pl.job_count[0] == (n > LIN_SMALL ? 0 : 1) && pl.small.size() == (n > LIN_SMALL ? 0u : 1u),
                  "%d pieces: job_count %d", n, (int)pl.job_count[0]);
        }
    }
    {   // 64 equal sequences fill a word: the mask of all ones
        std::vector<int32_t> labels(64, 0);
        std::vector<int64_t> V(64, 9);
        const LinPlan pl = build_lin_plan(labels.data(), V.data(), 64, 1, 64);
        CHECK(pl.pc_mask.size() == 1 && pl.pc_mask[0] == ~0ull && pl.pc_word[0] == 0 && pl.pc_v[0] == 9, "a full word is one piece");
    }
    printf("lin plan: done\n");
}

static void check_perm_order() {
    for (int32_t C : {1, 3, 70})
        for (int64_t N : {1, 64, 129, 500}) {
            std::vector<int32_t> labels((size_t)N);
            std::vector<int64_t> V((size_t)N);
            uint32_t x = (uint32_t)(N * 131 + C);
            int64_t P = 0;
            for (int64_t s = 0; s < N; ++s) {
                x = x * 1664525u + 1013904223u;
                labels[(size_t)s] = (int32_t)((x >> 10) % (uint32_t)(C + 1)) - 1;
                if (C >= 3 && labels[(size_t)s] == 1) labels[(size_t)s] = -1;   // an empty cluster
                V[(size_t)s] = 1000 - 3 * s;
                P += labels[(size_t)s] >= 0;
            }
            const PermOrder o = perm_order0(labels.data(), V.data(), N, C);
            CHECK((int64_t)o.order0.size() == P && (int64_t)o.v0.size() == P, "N %lld C %d: %zu of %lld", (long long)N, (int)C, o.order0.size(), (long long)P);
            bool sorted = true, follows = true;
            for (size_t p = 0; p < o.order0.size(); ++p) {
                const int32_t s = o.order0[p];
                if (s < 0 || s >= N || labels[(size_t)s] < 0) {
                    sorted = false;
                    break;
                }
                follows = follows && o.v0[p] == V[(size_t)s];
                if (p > 0) {
                    const int32_t r = o.order0[p - 1];
                    sorted = sorted && (labels[(size_t)r] < labels[(size_t)s] || (labels[(size_t)r] == labels[(size_t)s] && r < s));
                }
            }
            CHECK(sorted, "N %lld C %d: by label, by sequence within a label, every labelled sequence once", (long long)N, (int)C);
            CHECK(follows, "N %lld C %d: v0 follows order0", (long long)N, (int)C);
        }
    const std::vector<int32_t> none(10, -1);
    const std::vector<int64_t> V(10, 1);
    const PermOrder o = perm_order0(none.data(), V.data(), 10, 4);
    CHECK(o.order0.empty() && o.v0.empty(), "no labelled sequence");
    printf("perm order: done\n");
}

int main() {
    check_indices();
    check_labels();
    check_neff();
    check_distinct();
    check_budget();
    check_lin_plan();
    check_perm_order();
    printf("checks %d failures %d\n", checks, failures);
    return failures ? 1 : 0;
}

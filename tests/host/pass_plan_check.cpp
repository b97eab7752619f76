// Host check of the host-only parts of a pass over a block list — the SAME source the engine compiles (ldweaver_amd/csrc/ldw_pass_plan.h): the block
// descriptor rule, the plan (spans), the short-range pair count on the circle against brute force, and the hand-over between the helper threads
// and the submitting thread (PrepQueue) driven with a do-nothing prepare function.  Prints one line per group; exit code 0 iff nothing failed.
//   (tests/test_pass_plan_host.py builds it with g++ -O1 -std=c++17 -pthread and runs it; it is also the program to run under -fsanitize=thread)
#include <atomic>
#include <cstdio>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../ldweaver_amd/csrc/ldw_pass_plan.h"

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

// make_blocks (R/computePairwiseMI.R:147-165): block pairs (i, j >= i) of ranges of B SNPs, the last one ragged
static std::vector<int32_t> make_blocks(int32_t L, int32_t B) {
    std::vector<int32_t> s, e, out;
    for (int32_t a = 1; a <= L; a += B) {
        s.push_back(a);
        e.push_back(std::min(a + B - 1, L));
    }
    for (size_t i = 0; i < s.size(); ++i)
        for (size_t j = i; j < s.size(); ++j) out.insert(out.end(), {s[i], e[i], s[j], e[j]});
    return out;
}
static std::vector<int> span_sizes(const std::vector<WorkItem> &items) {
    std::vector<int> n;
    for (const WorkItem &it : items)
        if (it.nseg > 1) n.push_back(it.nseg);
    return n;
}
// items cover the blocks exactly once, in order
static bool covers(const std::vector<WorkItem> &items, int64_t nblocks) {
    int64_t b = 0;
    for (const WorkItem &it : items) {
        if (it.b0 != b || it.nseg < 1) return false;
        b += it.nseg;
    }
    return b == nblocks;
}
static std::string str(const std::vector<int> &v) {
    std::string s;
    for (int x : v) s += std::to_string(x) + " ";
    return s;
}

static void check_plan() {
    const int32_t B = 2048;
    const auto always = [](const int32_t *) { return true; };
    for (int ragged = 0; ragged < 2; ++ragged) {
        // positions 10 apart, sr_dist = half a block: a block pair is long-range only when a whole block lies between its sides, directly and across the origin
        const int32_t L = ragged ? 7 * B + 1000 : 8 * B;
        std::vector<int32_t> POS((size_t)L), bad((size_t)L + 1, 0);
        for (int32_t i = 0; i < L; ++i) POS[(size_t)i] = 10 * (i + 1);
        const SpanView v{L, 10.0 * L + 10.0, POS, bad, 5.0 * B};
        const auto lr_only = [&](const int32_t *b) { return span_candidate(v, b); };
        const std::vector<int32_t> blocks = make_blocks(L, B);
        const int64_t nb = (int64_t)blocks.size() / 4;
        CHECK(nb == 36, "%lld blocks", (long long)nb);
        const auto it8 = plan_items(blocks.data(), nb, true, 8, lr_only);
        // block row i holds the columns i + 2 .. 7 but for the pair that closes the circle — (0, 7), and with the short last column also (0, 6) — and
        // the ragged column itself, which is not square
        const std::vector<int> want8 = ragged ? std::vector<int>{4, 4, 3, 2} : std::vector<int>{5, 5, 4, 3, 2};
        CHECK(covers(it8, nb) && span_sizes(it8) == want8, "ragged %d nmax 8: spans %s", ragged, str(span_sizes(it8)).c_str());
        for (const WorkItem &it : it8)   // a span: candidates of one block row, to sides strictly ascending
            for (int q = 1; q < it.nseg; ++q) {
                const BlockRef a = BlockRef::at(blocks.data(), it.b0), p = BlockRef::at(blocks.data(), it.b0 + q - 1), d = BlockRef::at(blocks.data(), it.b0 + q);
                CHECK(lr_only(&blocks[(size_t)(it.b0 + q) * 4]) && d.fs == a.fs && d.fe == a.fe && d.ts > p.te, "span at block %lld", (long long)it.b0);
            }
        const auto it2 = plan_items(blocks.data(), nb, true, 2, lr_only);
        const std::vector<int> want2 = ragged ? std::vector<int>{2, 2, 2, 2, 2, 2} : std::vector<int>{2, 2, 2, 2, 2, 2, 2, 2};
        CHECK(covers(it2, nb) && span_sizes(it2) == want2, "ragged %d nmax 2: spans %s", ragged, str(span_sizes(it2)).c_str());
        const auto it1 = plan_items(blocks.data(), nb, true, 1, lr_only), it0 = plan_items(blocks.data(), nb, false, 8, lr_only);
        CHECK(covers(it1, nb) && (int64_t)it1.size() == nb && covers(it0, nb) && (int64_t)it0.size() == nb, "one item per block");
        // a SNP a span cannot hold (span_bad) takes its blocks out: SNP 3 B + 5 sits in block column 3
        bad.assign((size_t)L + 1, 0);
        for (int32_t i = 3 * B + 5; i <= L; ++i) bad[(size_t)i] = 1;
        const auto itb = plan_items(blocks.data(), nb, true, 8, lr_only);
        for (const WorkItem &it : itb)
            for (int q = 0; q < it.nseg && it.nseg > 1; ++q) {
                const BlockRef d = BlockRef::at(blocks.data(), it.b0 + q);
                CHECK(!(d.fs <= 3 * B + 5 && 3 * B + 5 <= d.fe) && !(d.ts <= 3 * B + 5 && 3 * B + 5 <= d.te), "a span holds the bad SNP");
            }
        CHECK(covers(itb, nb) && span_sizes(itb) != want8, "the bad SNP changes the plan");
    }
    {   // what breaks a span, with every block a candidate
        const int32_t asc[] = {1, 10, 11, 20, 1, 10, 21, 30, 1, 10, 31, 40};
        CHECK(span_sizes(plan_items(asc, 3, true, 8, always)) == std::vector<int>{3}, "ascending to sides form one span");
        const int32_t desc[] = {1, 10, 21, 30, 1, 10, 11, 20, 1, 10, 31, 40};
        const auto d = plan_items(desc, 3, true, 8, always);
        CHECK(covers(d, 3) && d.size() == 2 && d[0].nseg == 1 && d[1].nseg == 2, "a to side that does not ascend breaks the span");
        const int32_t same[] = {1, 10, 11, 20, 1, 10, 20, 29};   // (touching: te of the one == ts of the next)
        CHECK(plan_items(same, 2, true, 8, always).size() == 2, "to sides must ascend strictly");
        const int32_t from[] = {1, 10, 21, 30, 2, 11, 31, 40, 2, 11, 41, 50};
        const auto f = plan_items(from, 3, true, 8, always);
        CHECK(covers(f, 3) && f.size() == 2 && f[0].nseg == 1 && f[1].nseg == 2, "a different from side breaks the span");
        const int32_t from_e[] = {1, 10, 21, 30, 1, 11, 31, 40};
        CHECK(plan_items(from_e, 2, true, 8, always).size() == 2, "a different end of the from side breaks the span");
        const auto second_no = [](const int32_t *b) { return b[2] != 21; };
        const auto s = plan_items(asc, 3, true, 8, second_no);
        CHECK(covers(s, 3) && s.size() == 3, "a block that is no candidate breaks the span");
    }
    {   // the pair cap: 50 000 from-side SNPs, nf x nt_tot must stay BELOW 1.5e9 = 50 000 x 30 000
        const int32_t at[] = {1, 50000, 50001, 60000, 1, 50000, 60001, 70000, 1, 50000, 70001, 80000, 1, 50000, 80001, 90000};
        const auto a = plan_items(at, 4, true, 8, always);
        CHECK(covers(a, 4) && a.size() == 2 && a[0].nseg == 2 && a[1].nseg == 2, "the pair cap breaks the span at the segment that reaches it");
        const int32_t below[] = {1, 50000, 50001, 60000, 1, 50000, 60001, 70000, 1, 50000, 70001, 79999, 1, 50000, 80001, 90000};
        const auto b = plan_items(below, 4, true, 8, always);
        CHECK(covers(b, 4) && b.size() == 2 && b[0].nseg == 3 && b[1].nseg == 1, "one column fewer stays under the pair cap");
    }
    {   // the column cap: nt_tot <= 900 000 (1000 from-side SNPs: far from the pair cap)
        const int32_t at[] = {1, 1000, 1001, 301000, 1, 1000, 301001, 601000, 1, 1000, 601001, 901000, 1, 1000, 901001, 901001};
        const auto a = plan_items(at, 4, true, 8, always);
        CHECK(covers(a, 4) && a.size() == 2 && a[0].nseg == 3 && a[1].nseg == 1, "900 000 columns fit, one more does not");
        const int32_t over[] = {1, 1000, 1001, 301000, 1, 1000, 301001, 601000, 1, 1000, 601001, 901001, 1, 1000, 901002, 901002};
        const auto o = plan_items(over, 4, true, 8, always);
        CHECK(covers(o, 4) && o.size() == 2 && o[0].nseg == 2 && o[1].nseg == 2, "the column cap breaks the span at the segment that crosses it");
    }
    {   // the cold-start probe is expected from the FIRST off-diagonal block alone
        const int32_t bl[] = {1, 4000, 1, 4000, 1, 4000, 4001, 8000, 1, 4000, 8001, 8100};
        CHECK(probe_expected(bl, 3, 16000000) && !probe_expected(bl, 3, 16000001) && !probe_expected(bl, 1, 1) && !probe_expected(bl + 8, 1, 400001), "probe_expected");
        CHECK(total_pairs(bl, 3) == 4000.0 * 4000.0 * 2 + 4000.0 * 100.0, "total_pairs");
        CHECK(block_list_key(bl, 3, 20000.0) != block_list_key(bl, 2, 20000.0) && block_list_key(bl, 3, 20000.0) != block_list_key(bl, 3, 20000.5), "block_list_key");
    }
    {   // span_candidate at its geometric boundary: five blocks of 2048 SNPs one apart.  The nearest pair of (1, 3) is 2049 apart; (1, 5) closes the circle at g - 10239
        const int32_t L = 5 * B;
        std::vector<int32_t> POS((size_t)L), bad((size_t)L + 1, 0);
        for (int32_t i = 0; i < L; ++i) POS[(size_t)i] = i + 1;
        const int32_t b13[] = {1, B, 2 * B + 1, 3 * B}, b15[] = {1, B, 4 * B + 1, 5 * B}, b12[] = {1, B, B + 1, 2 * B};
        const auto cand = [&](const int32_t *b, double g, double sr) { return span_candidate(SpanView{L, g, POS, bad, sr}, b); };
        CHECK(cand(b13, 12288, 2048) && !cand(b13, 12288, 2049) && !cand(b12, 12288, 2048), "a pair at len == sr_dist keeps its block out of spans");
        CHECK(cand(b15, 12288, 2048) && !cand(b15, 12287, 2048) && cand(b15, 12287, 2047.5), "the same across the origin");
        CHECK(!cand(b13, 4096, 2048) && !cand(b13, 4097, 2048), "2 sr_dist >= g, and a genome shorter than the block's extent");
        // positions outside [0, g] or g and more apart: no block is a candidate, whatever its four end positions say
        CHECK(!within_one_turn(0, 10, 10) && within_one_turn(0, 9.5, 10) && within_one_turn(1, 10, 10) &&!within_one_turn(0, 11, 10) && !within_one_turn(-1, 5, 10) && !within_one_turn(0, 10, 9.5),
              "within_one_turn: all in [0, g], less than g apart");
        std::vector<int32_t> far(POS);
        for (int32_t &p : far) p += 20000;
        CHECK(cand(b13, 12288, 2048) && !span_candidate(SpanView{L, 12288, far, bad, 2048}, b13) && span_candidate(SpanView{L, 32288, far, bad, 2048}, b13),
              "positions beyond g: no span");
    }
    printf("plan: done\n");
}

static void check_descriptor() {
    const int64_t L = 100;
    const int32_t bad[][4] = {{0, 5, 1, 5}, {1, 101, 1, 5}, {1, 5, 0, 5}, {1, 5, 1, 101}, {6, 5, 1, 5}, {1, 5, 6, 5}};
    for (const auto &d : bad) {
        const BlockRef r = BlockRef::at(d, 0);
        CHECK(!r.in_range(L) && r.range_message(3, L).find("outside 1..100") != std::string::npos && r.range_message(3, L).find("block 3 = (") == 0,
              "(%d,%d,%d,%d): %s", d[0], d[1], d[2], d[3], r.range_message(3, L).c_str());
    }
    const int32_t good[][4] = {{1, 1, 1, 1}, {100, 100, 100, 100}, {1, 100, 1, 100}, {3, 7, 50, 100}};
    for (const auto &d : good) CHECK(BlockRef::at(d, 0).in_range(L), "(%d,%d,%d,%d) is in range", d[0], d[1], d[2], d[3]);
    const BlockRef r = BlockRef::at(good[3], 0);
    std::vector<int32_t> f, t{-1};
    r.append_from(f);
    r.append_to(t);
    CHECK(f == (std::vector<int32_t>{2, 3, 4, 5, 6}) && t.size() == 52 && t[0] == -1 && t[1] == 49 && t.back() == 99, "index lists are 0-based and appended");
    CHECK(!r.is_diag() && BlockRef::at(good[2], 0).is_diag() && r.nf() == 5 && r.nt() == 51 && r.pairs_of() == 255 && r.pairs_of_d() == 255.0, "sizes");
    const int32_t big[4] = {1, 1000000, 1000001, 2000000};   // (the int64 product: 1e12)
    CHECK(BlockRef::at(big, 0).pairs_of() == 1000000000000LL && BlockRef::at(big, 0).pairs_of_d() == 1e12, "pairs of a large block");
    printf("descriptor: done\n");
}

static int64_t sr_brute(const std::vector<int32_t> &P, double g, double d) {
    int64_t n = 0;
    for (size_t a = 0; a < P.size(); ++a)
        for (size_t b = a + 1; b < P.size(); ++b) n += ((double)P[b] - (double)P[a] <= d || (double)P[a] + g - (double)P[b] <= d) ? 1 : 0;
    return n;
}
static void check_sr_count() {
    // (g and d are multiples of 1/4 well below 2^50: every sum and difference here is exact, so the two spellings of the test across the origin agree)
    struct Case { std::vector<int32_t> P; double g, d; };
    std::vector<Case> cases = {
        {{7}, 100.0, 10.0}, {{7}, 100.0, 0.0},
        {{3, 9}, 100.0, 5.0}, {{3, 9}, 100.0, 6.0}, {{3, 98}, 100.0, 5.0}, {{3, 98}, 100.0, 4.0}, {{5, 5}, 100.0, 0.0}, {{1, 100}, 100.0, 1.0},
        {{1, 2, 3, 50, 51, 98, 99, 100}, 100.25, 3.25}, {{1, 2, 3, 50, 51, 98, 99, 100}, 100.25, 3.0},
    };
    std::mt19937 rng(1988);
    for (int k = 0; k < 12; ++k) {
        const int n = 150 + 37 * k;
        const int range = k % 3 == 0 ? n / 3 : (k % 3 == 1 ? 4 * n : 40 * n);   // many ties / some / hardly any
        std::vector<int32_t> P((size_t)n);
        for (auto &x : P) x = 1 + (int32_t)(rng() % (unsigned)range);
        std::sort(P.begin(), P.end());
        const double g = (double)range + (k % 2 ? 0.75 : 0.0) + (k % 4 == 0 ? 0.0 : 13.0);   // k % 4 == 0: the last position may sit at g itself
        for (double d : {0.0, 1.0, 7.25, g / 8, g / 2 - 0.25}) cases.push_back(Case{P, g, d});
    }
    int64_t across = 0, direct = 0;
    for (const Case &c : cases) {
        const int64_t want = sr_brute(c.P, c.g, c.d), got = sr_pairs_on_circle(c.P.data(), (int64_t)c.P.size(), c.g, c.d);
        CHECK(2 * c.d < c.g && want == got, "L %zu g %.2f d %.2f: %lld, brute force %lld", c.P.size(), c.g, c.d, (long long)got, (long long)want);
        const int64_t lin = sr_brute(c.P, 1e18, c.d);
        across += want - lin;
        direct += lin;
    }
    CHECK(across > 1000 && direct > 1000, "the cases hold pairs of both kinds (%lld direct, %lld across the origin)", (long long)direct, (long long)across);
    printf("short-range count: %zu cases, %lld pairs direct, %lld across the origin\n", cases.size(), (long long)direct, (long long)across);
}

// ---- the hand-over: 3 helpers, a ring of 8, 3 slots, as the engine runs it ----
constexpr int RING = 8, NSLOT = 3, HELPERS = 3;
struct Run {
    int64_t n;
    int64_t fail_at, fail_also;        // items whose preparation fails (-1: none)
    std::vector<int64_t> ring;         // what a helper "prepares": plain memory, ordered by the queue alone (a race here is the sanitizer's finding)
    std::unique_ptr<std::atomic<int>[]> times;   // per item: how often it was prepared
    std::atomic<int64_t> sub{0}, done{0};   // shadows of the two counters, stored BEFORE the queue learns of them: never behind it
    std::atomic<int64_t> violations{0};
    PrepQueue q;                       // last: joined before the ring goes
    Run(int64_t n_, int64_t fail_at_ = -1, int64_t fail_also_ = -1)
        : n(n_), fail_at(fail_at_), fail_also(fail_also_), ring(RING, -1), times(new std::atomic<int>[(size_t)n_]), q(n_, RING, NSLOT) {
        for (int64_t k = 0; k < n; ++k) times[(size_t)k] = 0;
    }
    void helper() {
        for (int64_t k; (k = q.take()) != PrepQueue::LEAVE;) {
            if (k >= done.load() + RING || k >= sub.load() + NSLOT || k < 0 || k >= n) ++violations;
            if (k == fail_at || k == fail_also) {
                q.failed(k, 40 + (int)(k - fail_at), "item " + std::to_string(k) + " failed");
                return;
            }
            ring[(size_t)(k % RING)] = k;
            ++times[(size_t)k];
            q.prepared(k);
        }
    }
    void start() { q.start(HELPERS, [this] { helper(); }); }
    void submitted(int64_t m) { sub.store(m), q.submitted(m); }
    void finished(int64_t m) { done.store(m), q.done(m); }
};

static void check_handover() {
    {   // a whole pass in the engine's order: item b + 1 is waited for, b + 2 is taken if it is ready, then item b is finished
        Run r(400);
        r.start();
        int rc = -1;
        std::string msg;
        int64_t n_sub = 0, wrong = 0;
        CHECK(r.q.wait_prepared(0, true, rc, msg) && rc == 0, "item 0");
        r.submitted(++n_sub);
        for (int64_t b = 0; b < r.n; ++b) {
            while (n_sub < r.n && n_sub <= b + NSLOT - 1) {
                const bool ready = r.q.wait_prepared(n_sub, n_sub == b + 1, rc, msg);
                if (rc != 0) ++wrong;
                if (!ready) break;
                r.submitted(++n_sub);
            }
            if (r.ring[(size_t)(b % RING)] != b) ++wrong;   // the entry is still item b's: nobody took item b + RING before b was finished
            r.finished(b + 1);
        }
        r.q.stop_and_join();
        int64_t not_once = 0;
        for (int64_t k = 0; k < r.n; ++k) not_once += r.times[(size_t)k] != 1;
        CHECK(wrong == 0 && not_once == 0 && r.violations == 0 && n_sub == r.n, "whole pass: %lld wrong, %lld items not prepared once, %lld taken too early", (long long)wrong,
              (long long)not_once, (long long)r.violations.load());
    }
    for (int64_t k : {(int64_t)0, (int64_t)150, (int64_t)299})
        for (int also = 0; also < 2; ++also) {   // also: the item behind it fails too — the lower one is reported
            if (also && k == 299) continue;
            Run r(300, k, also ? k + 1 : -1);
            r.start();
            int rc = -1;
            std::string msg;
            int64_t wrong = 0, j = 0;
            for (; j < r.n; ++j) {   // one item after the other, up to the failure
                const bool ready = r.q.wait_prepared(j, true, rc, msg);
                if (rc != 0) break;
                if (!ready || r.ring[(size_t)(j % RING)] != j) ++wrong;
                r.submitted(j + 1);
                r.finished(j + 1);
            }
            CHECK(j == k && wrong == 0 && rc == 40 && msg == "item " + std::to_string(k) + " failed", "failure at %lld (+%d): stopped at %lld, rc %d, '%s'", (long long)k, also,
                  (long long)j, rc, msg.c_str());
            r.q.stop_and_join();
            for (int64_t i = 0; i < r.n; ++i) {   // (wait = true must not block here: every item is prepared or behind the failure)
                msg.clear();
                const bool ready = r.q.wait_prepared(i, true, rc, msg);
                if (i < k ? !(ready && rc == 0 && msg.empty()) : !(rc == 40 && msg == "item " + std::to_string(k) + " failed")) ++wrong;
                // (another helper may have prepared an item or two behind the failed one before the failure was recorded)
                if (i <= k ? (r.times[(size_t)i] != (i < k ? 1 : 0) || ready != (i < k)) : (r.times[(size_t)i] > 1 || ready != (r.times[(size_t)i] == 1))) ++wrong;
            }
            CHECK(wrong == 0 && r.violations == 0, "failure at %lld (+%d): %lld wrong answers, %lld taken too early", (long long)k, also, (long long)wrong, (long long)r.violations.load());
        }
    {   // the lowest failed item is the one reported, in whichever order the failures arrive
        PrepQueue q(20, RING, NSLOT);
        int rc = -1;
        std::string msg;
        q.prepared(0);
        q.prepared(1);
        q.failed(5, 3, "five");
        CHECK(!q.wait_prepared(7, true, rc, msg) && rc == 3 && msg == "five" && !q.wait_prepared(4, false, rc, msg) && rc == 0, "one failure");
        q.failed(2, 4, "two");
        q.failed(9, 6, "nine");
        CHECK(!q.wait_prepared(2, true, rc, msg) && rc == 4 && msg == "two" && !q.wait_prepared(9, true, rc, msg) && rc == 4 && msg == "two", "the lower failure wins");
        CHECK(q.wait_prepared(1, true, rc, msg) && rc == 0 && q.take() == PrepQueue::LEAVE, "items before it stay good; a stopped queue hands nothing out");
    }
    {   // destruction with the helpers still waiting: nothing is ever submitted, so they stand at item NSLOT
        Run r(50);
        r.start();
        int rc = -1;
        std::string msg;
        CHECK(r.q.wait_prepared(NSLOT - 1, true, rc, msg) && rc == 0 && !r.q.wait_prepared(NSLOT, false, rc, msg), "the helpers wait at item %d", NSLOT);
    }
    {   // the ring alone holds the helpers back: 20 items submitted (the engine never runs that far ahead), none finished
        Run r(50);
        r.start();
        r.submitted(20);
        int rc = -1;
        std::string msg;
        CHECK(r.q.wait_prepared(RING - 1, true, rc, msg) && rc == 0 && !r.q.wait_prepared(RING, false, rc, msg), "the helpers wait at item %d", RING);
        r.finished(1);
        CHECK(r.q.wait_prepared(RING, true, rc, msg) && rc == 0, "item %d follows once item 0 is finished", RING);
        r.q.stop_and_join();
        CHECK(r.violations == 0 && r.times[RING + 1] == 0, "%lld items taken too early", (long long)r.violations.load());
    }
    {   // and with no item at all taken
        PrepQueue q(0, RING, NSLOT);
        q.start(HELPERS, [&q] { (void)q.take(); });
    }
    printf("hand-over: done\n");
}

int main() {
    check_descriptor();
    check_plan();
    check_sr_count();
    check_handover();
    printf("checks %d  failures %d\n", checks, failures);
    return failures ? 1 : 0;
}

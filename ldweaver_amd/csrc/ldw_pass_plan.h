// The host-only parts of a pass over a block list (ldw_mi_all_pairs, ldw_mi.hip / ldw_mi_pass.inc): the ONE rule of a block descriptor, the plan
// (which consecutive blocks form a span), the counts that size the link tables, and the hand-over between the helper threads that build the
// items' lists and the thread that submits them (PrepQueue).
// Plain C++, no HIP: tests/host/pass_plan_check.cpp reads this header with g++ (tests/test_pass_plan_host.py), also under a thread sanitizer.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace ldw {

// ------------------------------------------------------------------------------------------------
// a block descriptor: (fs, fe, ts, te), 1-based inclusive SNP ranges of the from side and the to side (make_blocks, R/computePairwiseMI.R:147-165)
// ------------------------------------------------------------------------------------------------
struct BlockRef {
    int32_t fs, fe, ts, te;
    static BlockRef at(const int32_t *blocks, int64_t b) { return BlockRef{blocks[b * 4 + 0], blocks[b * 4 + 1], blocks[b * 4 + 2], blocks[b * 4 + 3]}; }
    bool in_range(int64_t L) const { return fs >= 1 && fe >= fs && fe <= L && ts >= 1 && te >= ts && te <= L; }
    std::string range_message(int64_t b, int64_t L) const {
        char s[160];
        snprintf(s, sizeof(s), "block %lld = (%d,%d,%d,%d) outside 1..%lld", (long long)b, fs, fe, ts, te, (long long)L);
        return s;
    }
    bool is_diag() const { return fs == ts && fe == te; }
    int64_t nf() const { return (int64_t)(fe - fs + 1); }
    int64_t nt() const { return (int64_t)(te - ts + 1); }
    int64_t pairs_of() const { return nf() * nt(); }
    double pairs_of_d() const { return (double)(fe - fs + 1) * (double)(te - ts + 1); }
    // the 0-based index list of a side, appended to `out`
    static void append_side(int32_t s, int32_t e, std::vector<int32_t> &out) {
        for (int32_t k = s; k <= e; ++k) out.push_back(k - 1);
    }
    void append_from(std::vector<int32_t> &out) const { append_side(fs, fe, out); }
    void append_to(std::vector<int32_t> &out) const { append_side(ts, te, out); }
};

// the pairs of a block list (what a pass's tables are sized against) and its key: FNV-1a over the descriptors, seeded with sr_dist
inline double total_pairs(const int32_t *blocks, int64_t nblocks) {
    double n = 0;
    for (int64_t b = 0; b < nblocks; ++b) n += BlockRef::at(blocks, b).pairs_of_d();
    return n;
}
inline uint64_t block_list_key(const int32_t *blocks, int64_t nblocks, double sr_dist) {
    uint64_t key = 1469598103934665603ull ^ (uint64_t)(int64_t)(sr_dist * 16.0);
    for (int64_t b = 0; b < nblocks; ++b)
        for (int q = 0; q < 4; ++q) key = (key ^ (uint64_t)(uint32_t)blocks[b * 4 + q]) * 1099511628211ull;
    return key;
}

// an off-diagonal guess can be sampled: the FIRST off-diagonal block of the list is large enough for the cold-start probe
inline bool probe_expected(const int32_t *blocks, int64_t nblocks, int64_t min_pairs) {
    for (int64_t b = 0; b < nblocks; ++b) {
        const BlockRef d = BlockRef::at(blocks, b);
        if (!d.is_diag()) return d.pairs_of() >= min_pairs;
    }
    return false;
}

// ------------------------------------------------------------------------------------------------
// One turn of the circle.  Every shortcut of the short/long-range split that works on POSITION WINDOWS or on a block's end positions (build_cols'
// three windows and its quick reject, k_cols_dev, span_candidate, the rejects of ldw_sr_pairs_fill) assumes that the positions of the block's two
// sides lie within one turn: all in [0, g] and less than g apart.  The difference of two such positions lies in (-g, g), where "within sr_dist
// on the circle" IS the union of the three windows.  The reference accepts any positions (its %% folds them), and ldw_set_snp_meta does not
// bound POS by g: a block outside this condition takes the predicate itself, pair by pair, everywhere.
// ------------------------------------------------------------------------------------------------
inline bool within_one_turn(double p_min, double p_max, double g) { return p_min >= 0 && p_max <= g && p_max - p_min < g; }

// ------------------------------------------------------------------------------------------------
// spans (r04): which blocks of the list may share a launch sequence
// ------------------------------------------------------------------------------------------------
// A block can be part of a span when its to side lies strictly AFTER its from side (make_blocks order: i < j), it is square, far enough
// from its from side that no pair is short-range (POS ascends over the alignment: the test of build_cols on the four end positions), and
// neither side holds a SNP the fused table test cannot place (no indicator row, or unflagged slots: span_bad, a prefix count over 1..L).
// Corner blocks (a few short-range pairs at the facing ends) stay items of their own: docs/HISTORY.md 6b.
struct SpanView {   // what span_candidate reads of the context and the call
    int64_t L;
    double g;
    const std::vector<int32_t> &POS, &span_bad;
    double sr_dist;
};
inline bool span_candidate(const SpanView &v, const int32_t *b) {
    const int64_t fs = b[0], fe = b[1], ts = b[2], te = b[3];
    if (!(fs >= 1 && fe >= fs && ts > fe && te >= ts && te <= v.L)) return false;
    const int64_t nf = fe - fs + 1, nt = te - ts + 1;
    if (nf != nt || nf < 2048) return false;
    if ((int64_t)v.span_bad.size() != v.L + 1) return false;
    if (v.span_bad[(size_t)fe] - v.span_bad[(size_t)fs - 1] != 0 || v.span_bad[(size_t)te] - v.span_bad[(size_t)ts - 1] != 0) return false;
    if (!(2 * v.sr_dist < v.g)) return false;
    const std::vector<int32_t> &P = v.POS;
    const double pf_min = P[(size_t)fs - 1], pf_max = P[(size_t)fe - 1], pt_min = P[(size_t)ts - 1], pt_max = P[(size_t)te - 1];
    if (!within_one_turn(pf_min, pt_max, v.g)) return false;   // (POS ascends and ts > fe: the block's smallest and largest position)
    return pt_min - pf_max > v.sr_dist && pf_min + v.g - pt_max > v.sr_dist;
}

struct WorkItem {
    int64_t b0;
    int nseg;           // 1: an ordinary block
};
constexpr int64_t SPAN_PAIRS_CAP = 1500000000LL;   // nf x nt of a span stays below the 32-bit index limit of the unit lists
constexpr int64_t SPAN_COLS_CAP = 900000;          // and its int32 block below ~6 GB

// The items of a pass, in block order: consecutive candidates of one block row (same from side), to sides strictly ascending, form a span
// of at most nmax blocks within the two caps; every other block is an item of its own.
template <class Candidate> std::vector<WorkItem> plan_items(const int32_t *blocks, int64_t nblocks, bool spans, int nmax, Candidate candidate) {
    std::vector<WorkItem> items;
    for (int64_t b = 0; b < nblocks;) {
        int n = 1;
        if (spans && candidate(blocks + b * 4)) {
            const BlockRef first = BlockRef::at(blocks, b);
            int64_t nt_tot = first.nt();
            while (n < nmax && b + n < nblocks && candidate(blocks + (b + n) * 4)) {
                const BlockRef d = BlockRef::at(blocks, b + n);
                if (d.fs != first.fs || d.fe != first.fe || !(d.ts > blocks[(b + n - 1) * 4 + 3])) break;
                if (first.nf() * (nt_tot + d.nt()) >= SPAN_PAIRS_CAP || (nt_tot + d.nt()) > SPAN_COLS_CAP) break;
                nt_tot += d.nt();
                ++n;
            }
        }
        items.push_back(WorkItem{b, n});
        b += n;
    }
    return items;
}

// ------------------------------------------------------------------------------------------------
// The number of SNP pairs within sr_dist on the circle of length g (needs 2 sr_dist < g, POS ascending): it bounds the short-range rows of a
// pass, whose blocks hold every unordered pair at most once.  A two-pointer walk, O(L) (r03 ran build_cols over every block for this, 0.2 ms
// each, and only for passes of more than 200 blocks).
// ------------------------------------------------------------------------------------------------
inline int64_t sr_pairs_on_circle(const int32_t *P, int64_t L, double g, double sr_dist) {
    int64_t total = 0, hi = 0, wlo = 0;
    for (int64_t a = 0; a < L; ++a) {
        if (hi < a + 1) hi = a + 1;
        while (hi < L && (double)P[(size_t)hi] - (double)P[(size_t)a] <= sr_dist) ++hi;
        total += hi - a - 1;                                   // partners ahead of a, directly
    }
    for (int64_t a = 0; a < L; ++a) {   // partners across the origin: b before a with P[b] + g - P[a] <= sr_dist (the limit ascends with a)
        const double lim = sr_dist - g + (double)P[(size_t)a];
        if (lim < (double)P[0]) continue;
        while (wlo < L && (double)P[(size_t)wlo] <= lim) ++wlo;
        total += std::min<int64_t>(wlo, a);
    }
    return total;
}

// ------------------------------------------------------------------------------------------------
// The prep hand-over.  Helper threads build the lists of the items (prep_block: pure host work into a slot's pinned staging buffer) ahead of
// the thread that submits them; item k lives in entry k % ring of a ring of HostBlocks and uses pipeline slot k % nslot.  Two conditions let a
// helper take item k:
//     k < n_done + ring     item k - ring is finished: its ring entry is free
//     k < n_sub + nslot     item k - nslot has been submitted: the slot's staging buffer belongs to an upload the helper can wait for (ev_up)
// The helpers take the items in order, so when the preparation of item k fails every item before k is prepared or being prepared: the pass
// runs on to the failed item itself, like the reference's loop (R/computePairwiseMI.R:103-116) — a failure does not concern an earlier item.
// The mutex guards every data member below except the threads; nothing outside the class touches them.
// Two lifetime facts its user keeps (ItemLoop, ldw_mi_pass.inc): the ring the worker writes to is declared BEFORE the queue and so outlives
// the join of the destructor; whatever the worker reads of the pass's state (ldw_ctx::early_sr) is stored before start().
// ------------------------------------------------------------------------------------------------
class PrepQueue {
  public:
    static constexpr int64_t LEAVE = -1;
    PrepQueue(int64_t nitems, int ring, int nslot) : nitems_(nitems), ring_(ring), nslot_(nslot), prepped_((size_t)nitems + 1, 0) {}
    ~PrepQueue() { stop_and_join(); }   // every way out of a pass stops and joins the helpers

    template <class Worker> void start(int n_helpers, Worker worker) {
        for (int i = 0; i < n_helpers; ++i) helpers_.emplace_back(worker);
    }
    // a helper's wait: the next item, or LEAVE (stopped, or nothing left)
    int64_t take() {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return stop_ || next_ >= nitems_ || (next_ < n_done_ + ring_ && next_ < n_sub_ + nslot_); });
        return (stop_ || next_ >= nitems_) ? LEAVE : next_++;
    }
    void prepared(int64_t k) { tell([&] { prepped_[(size_t)k] = 1; }); }
    // keeps the failure of the LOWEST item (helpers finish out of order) and stops the helpers
    void failed(int64_t k, int rc, const std::string &msg) {
        tell([&] {
            if (rc_ == 0 || k < bad_) rc_ = rc, err_ = msg;
            bad_ = std::min(bad_, k);
            stop_ = true;
        });
    }
    // blocks until item k is prepared or failed (wait = false: only says how things stand).  true: prepared.  rc / msg: the recorded failure
    // when it is item k's or an earlier item's, else 0.
    bool wait_prepared(int64_t k, bool wait, int &rc, std::string &msg) {
        std::unique_lock<std::mutex> lk(m_);
        if (wait) cv_.wait(lk, [&] { return (rc_ != 0 && k >= bad_) || prepped_[(size_t)k] != 0; });
        rc = (rc_ != 0 && k >= bad_) ? rc_ : 0;
        if (rc != 0) msg = err_;
        return prepped_[(size_t)k] != 0;
    }
    void submitted(int64_t n) { tell([&] { n_sub_ = n; }); }   // items [0, n) have been submitted
    void done(int64_t n) { tell([&] { n_done_ = n; }); }       // items [0, n) are finished
    void stop_and_join() {
        tell([&] { stop_ = true; });
        for (std::thread &t : helpers_)
            if (t.joinable()) t.join();
    }

  private:
    template <class Change> void tell(Change change) {   // a change of the shared state under the mutex, then everybody looks again
        {
            std::lock_guard<std::mutex> lk(m_);
            change();
        }
        cv_.notify_all();
    }
    const int64_t nitems_;
    const int ring_, nslot_;
    std::mutex m_;
    std::condition_variable cv_;
    int64_t n_sub_ = 0, n_done_ = 0, next_ = 0;   // next_: the item the next free helper takes
    std::vector<uint8_t> prepped_;                // per item (helpers finish out of order)
    int rc_ = 0;
    int64_t bad_ = INT64_MAX;                     // the first item whose preparation failed (items before it are still good: r05)
    bool stop_ = false;
    std::string err_;
    std::vector<std::thread> helpers_;
};

}  // namespace ldw

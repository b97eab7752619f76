// Part of ldw_mi.hip (inside its anonymous namespace): the parts of a PASS over a block list, in the order ldw_mi_all_pairs runs them — the plan
// (ldw_pass_plan.h, with what it needs of the context), the helper threads' body, the sizing of the link tables, the cold-start probes and the
// item loop with its failure drain.  The phases of an item (prep_block, submit_a / submit_b / finish_block) are in ldw_mi_items.inc.

// the one range check of a block descriptor, as an error of the C ABI
static int check_block(const ldw_ctx *c, const int32_t *blocks, int64_t b) {
    const BlockRef d = BlockRef::at(blocks, b);
    LDW_REQUIRE(d.in_range(c->L), LDW_ERR_ARG, "%s", d.range_message(b, c->L).c_str());
    return LDW_OK;
}

// ---- the plan ----
// what the whole pass must offer for spans (checked once, when the pass is planned: a positive guess for off-diagonal blocks exists, or — guess_expected —
// the cold-start probe of the pass is about to sample one)
static bool spans_possible(const ldw_ctx *c, const ldw_mi_params *p, bool guess_expected) {
    static const bool env_off = getenv("LDW_NO_SPAN") != nullptr;
    return c->knobs.span_on && !env_off && c->knobs.span_max >= 2 && c->knobs.prune && c->knobs.engine == LDW_ENGINE_MFMA && c->apx.apx_ok && c->knobs.path_mode != 1 && c->knobs.screen == 1 &&
           !p->sr_only && speculation_pays(c, p) && c->meta.pos_sorted && (c->spec.spec_B_next[0] > 0 || guess_expected) &&
           (p->quirk_mode != LDW_QUIRK_REFERENCE || c->meta.r_min >= 2.0);
}
static int span_nmax(const ldw_ctx *c) {
    static const int env_max = [] { const char *e = getenv("LDW_SPAN_MAX"); return e ? atoi(e) : 0; }();   // (A/B measurements)
    return std::min<int>(env_max >= 1 ? env_max : c->knobs.span_max, LDW_SPAN_MAX);
}
// The plan: items in block order, made BEFORE the helpers start and before the cold-start probes are queued, so that the list building of
// the first span (~3 ms for eight blocks, against 1.3 ms of GPU work in the diagonal block in front of it) runs beside the probes and
// the first item instead of after them.  Whether spans may form depends on a positive guess for off-diagonal blocks: on a cold pass the
// plan ASSUMES the off-diagonal probe will deliver one (it is known here whether that probe will be attempted).  A probe that then
// yields no guess costs time, never a row: the spans planned on it fall back as any span whose guess has gone does (submit_a: span_alone).
struct PassPlan {
    bool probes_wanted = false;
    bool spans = false;            // the pass may hold spans: it assigns short-range rows at submit time (ldw_ctx::early_sr)
    std::vector<WorkItem> items;
};
static PassPlan plan_pass(const ldw_ctx *c, const int32_t *blocks, int64_t nblocks, const ldw_mi_params *p) {
    static const bool probe_on = getenv("LDW_NO_PROBE") == nullptr;
    PassPlan plan;
    plan.probes_wanted = probe_on && !p->sr_only && c->meta.pos_sorted && speculation_pays(c, p);
    // an off-diagonal guess is missing and the first off-diagonal block is large enough to be sampled
    const bool guess_expected = plan.probes_wanted && c->spec.spec_B_next[0] < 0 && probe_expected(blocks, nblocks, PROBE_MIN_PAIRS);
    plan.spans = spans_possible(c, p, guess_expected);
    const SpanView v{c->L, c->meta.g, c->meta.h_POS, c->rows.h_span_bad, p->sr_dist};
    plan.items = plan_items(blocks, nblocks, plan.spans, plan.spans ? span_nmax(c) : 1, [&](const int32_t *b) { return span_candidate(v, b); });
    return plan;
}

// ---- table sizing ----
// Runs AFTER the helpers have started: it then lies beside the list building of the first items, which is what the GPU waits for.
static int size_link_tables(ldw_ctx *c, const int32_t *blocks, int64_t nblocks, const ldw_mi_params *p) {
    const double tot_pairs = total_pairs(blocks, nblocks);
    if (p->keep_sr && c->meta.pos_sorted && 2 * p->sr_dist < c->meta.g) {
        // Size the short-range table ONCE: geometric growth re-copies up to a gigabyte and synchronises both streams every time (ten times in
        // the first pass of C4), and would double-buffer tens of GB at C5.  The pairs within sr_dist on the circle bound the rows
        // (sr_pairs_on_circle: 1 ms at L = 100k, so once per positions and sr_dist).
        if (!(c->sizing.sr_total_dist == p->sr_dist && c->sizing.sr_total >= 0)) {
            c->sizing.sr_total = sr_pairs_on_circle(c->meta.h_POS.data(), c->L, c->meta.g, p->sr_dist);
            c->sizing.sr_total_dist = p->sr_dist;
        }
        const int64_t total_sr = c->sizing.sr_total;
        // r05: a SHARE of the block list (a rank or context of a multi-GPU job: under three quarters of the pair space) is sized for the rows of ITS blocks — the band
        // enumerator counts them on the device in well under a millisecond (ldw_sr_pairs_fill without outputs; cached per block list) — instead of the whole alignment's:
        // at config 5 that is 4.5 instead of 36 GB per rank of eight.  Whatever this under-estimates still grows where it is used (ensure_links_capacity per item).
        int64_t want_sr = total_sr;
        if (tot_pairs < 0.375 * (double)c->L * (double)c->L && c->meta.g == std::floor(c->meta.g)) {
            const uint64_t key = block_list_key(blocks, nblocks, p->sr_dist);
            if (c->sizing.sr_share_rows >= 0 && c->sizing.sr_share_key == key) want_sr = std::min(total_sr, c->sizing.sr_share_rows);
            else {
                int64_t n_share = 0;
                if (ldw_sr_pairs_fill(c, blocks, nblocks, p->sr_dist, nullptr, nullptr, 0, &n_share) == LDW_OK && n_share <= total_sr) {
                    c->sizing.learn_share(key, n_share);
                    want_sr = n_share;
                }
            }
        }
        if (int rc = ensure_links_capacity(c, want_sr + 1024, 0)) return rc;
    }
    if (!p->sr_only) {
        // r05: the long-range table sized ONCE as well.  The per-block filter keeps about lr_retain_links rows in all (R/computePairwiseMI.R:347-358:
        // prob = 1 - lr_retain_links / lr_links_approx), and what a selection needs beyond the rows kept so far is its own candidate count (<= 2^20 on
        // the sort-free path): 1.25 lr_retain_links + 4 M rows, at most the pass's pairs.  A fresh context grew the table nine times in its first
        // pass — each time a stream synchronisation, and with lr_links.tsv streaming (ldw_lr_stream_begin) a wait for the writer thread on top
        // (tools/lr_stream_probe.py: first pass 72-88 ms against 41).  Whatever this under-estimates still grows where it is used.
        const double want = std::min(tot_pairs, std::max(0.0, p->lr_retain_links) * 1.25 + (double)(4 << 20));
        if (want < 4e9)
            if (int rc = ensure_links_capacity(c, c->links.n_sr, (int64_t)want)) return rc;
    }
    return LDW_OK;
}

// ---- the cold-start probes: a sampled guess for each block kind that has none yet (probe_kind_guess), taken from the first block of the kind ----
struct Probes {
    Probe probe[2];
    int n = 0;
    int deferred = -1;   // the probe still to collect
};
static int queue_probes(ldw_ctx *c, const int32_t *blocks, int64_t nblocks, const ldw_mi_params *p, const SmallLayout &sl, Probes &pr) {
    bool done_kind[2] = {false, false};
    size_t pin_base = 0;
    std::vector<int32_t> fi, ti;
    for (int64_t b = 0; b < nblocks && !(done_kind[0] && done_kind[1]); ++b) {
        const BlockRef d = BlockRef::at(blocks, b);
        const int kind = d.is_diag() ? 1 : 0;
        if (done_kind[kind]) continue;
        done_kind[kind] = true;
        if (c->spec.spec_B_next[kind] >= 0) continue;
        if (int rc = check_block(c, blocks, b)) return rc;
        const int64_t npairs = d.is_diag() ? d.nf() * (d.nf() - 1) / 2 : d.pairs_of();
        if (npairs < PROBE_MIN_PAIRS) continue;
        fi.clear();
        ti.clear();
        d.append_from(fi);
        d.append_to(ti);
        // (a staging buffer that has to grow for the second sample is reallocated: the first sample's upload must have left it)
        if (pr.n > 0 && c->pin[LDW_NSLOT].cap < pin_base + 2 * pr.probe[0].hb.total + 65536) LDW_HIP(hipStreamSynchronize(c->stream));
        if (int rc = probe_enqueue(c, fi.data(), (int64_t)fi.size(), ti.data(), (int64_t)ti.size(), p, sl, kind, pr.n, pin_base, pr.probe[pr.n])) return rc;
        pin_base = (pin_base + pr.probe[pr.n].hb.total + 255) / 256 * 256;
        ++pr.n;
    }
    return LDW_OK;
}
// The host waits for the probes the first item needs — the one that ran on slot 0's buffers, the one of the item's own kind — and NOT for a
// second probe of the other kind: that one finishes on the main stream beside the item's block-wide pass and is collected behind the item's
// second phase, before anything else is submitted (collect_deferred).
static int collect_probes_for(ldw_ctx *c, const HostBlock &first, Probes &pr) {
    const int kind0 = first.diag ? 1 : 0;
    for (int k = 0; k < pr.n; ++k) {
        if (!pr.probe[k].queued) continue;
        if (pr.probe[k].which != 0 && pr.probe[k].kind != kind0) {
            pr.deferred = k;
            continue;
        }
        LDW_HIP(hipEventSynchronize(c->ev_probe[pr.probe[k].which]));
        probe_collect(c, pr.probe[k]);
    }
    return LDW_OK;
}
static int collect_deferred(ldw_ctx *c, Probes &pr) {
    if (pr.deferred < 0) return LDW_OK;
    LDW_REQUIRE(hipEventSynchronize(c->ev_probe[pr.probe[pr.deferred].which]) == hipSuccess, LDW_ERR_HIP, "cold-start probe: hipEventSynchronize failed");
    probe_collect(c, pr.probe[pr.deferred]);
    pr.deferred = -1;
    return LDW_OK;
}

// ---- the item loop ----
// Software pipeline, three ITEMS deep on the host (an item = one block, or a span of consecutive long-range-only blocks of one block
// row: r04): item i's epilogue chain is submitted (main stream), then at once the block-wide pass of item i+1 (GEMM stream; prepared
// earlier), and only then the host waits for item i's pick(s).
// r03: the lists of an item are built by a HELPER THREAD that runs ahead of the submitting thread (prep_block is pure host work into the
// slot's pinned staging buffer: 0.45 ms per 10k x 10k block — once the GPU side of a block had come down to 0.5 ms it was the loop's
// critical path).  The hand-over is PrepQueue's (ldw_pass_plan.h).  The plan is complete before the helpers start; the GEMM stream runs up
// to LDW_NSLOT - 1 = 2 items ahead of the item the main stream evaluates.
// r04: TWO helpers (a span of eight blocks took ~3 ms of list building, a diagonal block in front of it gives the
// GPU 1.3 ms of work: one helper left the GEMM stream waiting).  Each takes the next item; items k, k+1, k+2 use different slots.
// Now one helper per slot: with the whole plan known at the start, the first three items — the diagonal block, the corner block next
// to it and the first span (1.2, 0.9 and 2 ms of list building) — are prepared side by side, where the span used to start behind the
// corner block and the GEMM stream stood idle for 0.4-0.9 ms in front of it (profiles/cold_start_timeline.txt).
struct ItemLoop {
    static constexpr int RING = 8;
    ldw_ctx *c;
    const int32_t *blocks;
    const ldw_mi_params *p;
    const SmallLayout &sl;
    const std::vector<WorkItem> &items;
    const int64_t nitems;
    HostBlock hb[RING];
    int64_t n_sub = 0;            // items [0, n_sub) have been submitted to the GEMM stream
    double th[4] = {0, 0, 0, 0};  // host microseconds of the loop's four steps
    int fail_rc = LDW_OK;         // the first failure of the loop ...
    std::string fail_msg;
    int64_t b_fail = -1;          // ... and the item the loop was at when it failed
    bool b_fail_submitted = false, b_fail_finished = false;
    PrepQueue q;                  // LAST member: its destructor joins the helpers while the ring they write to is still there

    ItemLoop(ldw_ctx *c_, const int32_t *blocks_, const ldw_mi_params *p_, const SmallLayout &sl_, const std::vector<WorkItem> &items_)
        : c(c_), blocks(blocks_), p(p_), sl(sl_), items(items_), nitems((int64_t)items_.size()), q(nitems, RING, LDW_NSLOT) {}
    void start_helpers() {   // (the plan and c->early_sr are final here)
        q.start(LDW_NSLOT, [this] { helper(); });
    }
    int prep_item(int64_t k, std::vector<int32_t> &fi, std::vector<int32_t> &ti);
    void helper();
    int wait_prepared(int64_t k, bool wait = true, bool *ready = nullptr);
    int submit_next();
    int run(Probes &pr);
    int drain_after_failure();
    int failed(int rc, int64_t b, bool sub_b, bool fin) {
        fail_rc = rc;
        fail_msg = ldw_last_error();
        b_fail = b;
        b_fail_submitted = sub_b;
        b_fail_finished = fin;
        return rc;
    }
    void finished(int64_t b) {   // item b's rows are in the tables
        c->links.blk_cursor += items[(size_t)b].nseg;
        lr_stream_push(c, c->stream, sl.lr_count, c->links.blk_cursor);   // (no-op without ldw_lr_stream_begin: the rows of this item may go to lr_links.tsv now)
    }
};

// the helper's work on item k: its index lists, the wait for the slot's staging buffer, prep_block into ring entry k % RING
int ItemLoop::prep_item(int64_t k, std::vector<int32_t> &fi, std::vector<int32_t> &ti) {
    const WorkItem it = items[(size_t)k];
    try {   // (prep_block allocates a dozen std::vectors: an exception on this thread must come back as an error code, not std::terminate)
        SpanPlan spn;
        fi.clear();
        ti.clear();
        for (int s = 0; s < it.nseg; ++s) {
            if (int rc = check_block(c, blocks, it.b0 + s)) return rc;
            const BlockRef d = BlockRef::at(blocks, it.b0 + s);
            spn.start[s] = (int32_t)ti.size();
            spn.nt[s] = (int32_t)d.nt();
            d.append_to(ti);
        }
        spn.nseg = it.nseg;
        BlockRef::at(blocks, it.b0).append_from(fi);
        const int slot = (int)(k % LDW_NSLOT);
        LDW_REQUIRE(!c->up_recorded[slot] || hipEventSynchronize(c->ev_up[slot]) == hipSuccess, LDW_ERR_HIP, "prep: hipEventSynchronize failed");   // the staging buffer of this slot has been uploaded
        HostBlock &h = hb[k % RING];
        if (int rc = prep_block(c, fi.data(), (int64_t)fi.size(), ti.data(), (int64_t)ti.size(), p, slot, it.b0, h, it.nseg > 1 ? &spn : nullptr)) return rc;
        if (it.nseg > 1) {
            h.span_from = fi;
            h.span_to = ti;
        }
        return LDW_OK;
    } catch (const std::exception &e) {
        set_error("preparing block %lld: %s", (long long)it.b0, e.what());
    } catch (...) {
        set_error("preparing block %lld: unknown exception", (long long)it.b0);
    }
    return LDW_ERR_HIP;
}
void ItemLoop::helper() {
    (void)hipSetDevice(c->device);
    std::vector<int32_t> fi, ti;   // this helper's own index lists
    for (int64_t k; (k = q.take()) != PrepQueue::LEAVE;) {
        const int rc = prep_item(k, fi, ti);
        if (rc != LDW_OK) {
            q.failed(k, rc, ldw_last_error());
            return;
        }
        q.prepared(k);
    }
}

// blocks until item k is prepared — or, with wait = false, says in *ready whether it is; the error is a failure of item k or of an earlier one
int ItemLoop::wait_prepared(int64_t k, bool wait, bool *ready) {
    int rc = LDW_OK;
    std::string msg;
    const bool is = q.wait_prepared(k, wait, rc, msg);
    if (ready) *ready = is;
    if (rc != LDW_OK) set_error("%s", msg.c_str());
    return rc;
}
int ItemLoop::submit_next() {
    if (int rc = submit_a(c, hb[n_sub % RING], p, sl)) return rc;
    q.submitted(++n_sub);
    return LDW_OK;
}

int ItemLoop::run(Probes &pr) {
    const int64_t ahead = c->knobs.overlap ? LDW_NSLOT - 1 : 1;
    for (int64_t b = 0; b < nitems; ++b) {
        HostBlock &cur = hb[b % RING];
        HostClock::Point t0 = HostClock::now();
        if (int rc = submit_b(c, cur, p, sl)) return failed(rc, b, false, false);   // epilogue + pick of item b (main stream)
        th[0] += HostClock::us(t0, HostClock::now());
        // (b == 0) the probe of the other kind ran in front of this second phase: its guess is there before any item of its kind is submitted
        if (int rc = collect_deferred(c, pr)) return failed(rc, b, true, false);
        t0 = HostClock::now();
        // items b+1 .. b+ahead (GEMM stream) run beside them: b+1 is waited for, the ones after it are taken if they are ready
        while (n_sub < nitems && n_sub <= b + ahead) {
            bool ready = false;
            const HostClock::Point tw = HostClock::now();
            const int rc = wait_prepared(n_sub, n_sub == b + 1, &ready);
            th[1] += HostClock::us(tw, HostClock::now());
            if (rc) return failed(rc, b, true, false);
            if (!ready || !can_submit_early(c, hb[n_sub % RING], p)) break;
            if (int rc2 = submit_next()) return failed(rc2, b, true, false);
        }
        th[2] += HostClock::us(t0, HostClock::now());
        t0 = HostClock::now();
        // (tried: the second phase of block b+1 queued HERE, before the host waits for block b's pick, so that the main stream has work during the
        // round trip — block b's selection then runs behind it, its slot is released later, and the pass got slower: 43.0 against 40.2 ms)
        if (int rc = finish_block(c, cur, p, sl)) return failed(rc, b, true, false);   // round trip + selection of item b
        th[3] += HostClock::us(t0, HostClock::now());
        q.done(b + 1);
        finished(b);
        if (n_sub <= b + 1 && b + 1 < nitems) {                          // overlap off / no guess yet: one item after the other
            if (int rc = wait_prepared(b + 1)) return failed(rc, b, true, true);
            if (int rc = submit_next()) return failed(rc, b, true, true);
        }
    }
    return LDW_OK;
}

// r05: with lr_links.tsv streaming, the items that were submitted before the failure are run to their end, so that the file holds
// the rows of EVERY block in front of the failed one — what the reference's loop has appended when it stops at a block (:362).
// Best effort: a second failure in here is ignored, the first one is reported.
int ItemLoop::drain_after_failure() {
    if (c->lr_stream && b_fail >= 0) {
        for (int64_t bb = b_fail; bb < n_sub; ++bb) {
            HostBlock &h = hb[bb % RING];
            if (bb == b_fail && b_fail_finished) continue;
            if (!(bb == b_fail && b_fail_submitted))
                if (submit_b(c, h, p, sl) != LDW_OK) break;
            if (finish_block(c, h, p, sl) != LDW_OK) break;
            finished(bb);
        }
    }
    set_error("%s", fail_msg.c_str());
    return fail_rc;
}

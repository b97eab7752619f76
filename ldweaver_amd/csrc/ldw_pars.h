// What ldw_pars.hip lends to the other unit that runs the parsimony passes (ldw_coscan.hip): the checked tree, the working memory of a call and the
// chunked run of the passes.  Everything is defined in ldw_pars.hip; the kernels stay there.
#pragma once
#include <functional>
#include <vector>

#include "ldw_internal.h"

namespace ldw {

// the tree as the kernels read it, checked: nothing here touches the device
struct ParsTree {
    int64_t nodes = 0, tips = 0;
    std::vector<int32_t> child_ptr, child_idx;   // CSR: the children of v in ascending order
    std::vector<int32_t> tip_seq, tip_node;      // the tips in ascending order of their sequence
};

struct ParsBufs {   // the working memory of one call (the entry points release it)
    DevBuf sets, seen, score, minch, parent, child_ptr, child_idx, tip_seq, tip_node, snp, bits, state, slot_a, slot_b, ca, cb, co;
};

// what section (17) of the header refuses of a tree, under the caller's name
int pars_check_tree(const ldw_ctx *c, const char *who, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, ParsTree &t);

// What the entry points share: the tree on the device, then chunk after chunk of `total` SNP slots (slot j is SNP snp[j], or SNP j where snp is null)
// the tips, the up pass and, with `down`, the down pass; after_chunk(first slot, count) queues what the caller wants of the chunk's sets before the next
// chunk overwrites them.  ldw_ctx_last_timing: [0] the passes, [1] the gathers, [2] whatever after_chunk and the caller queued behind, [3] their sum.
struct ParsRun {
    ldw_ctx *c;
    ParsBufs &b;
    const ParsTree &t;
    int32_t gap_mode;
    int64_t C = 0, Cpad = 0, stride4 = 0;
    Laps laps;   // three events per chunk and one behind the last

    int start(const int32_t *parent, int64_t total, const int32_t *snp, bool want_score, bool down);
    int chunks(int64_t total, bool have_snp, bool want_score, bool down, uint32_t *bits, int64_t bit_stride, const std::function<int(int64_t, int64_t)> &after_chunk);
    int lap_sums(double ms[3]) const { return laps.sums(3, ms); }   // after the stream has drained: [0] the gathers, [1] the passes, [2] what followed a chunk
    int finish();                                                   // ... into the context's timing slots
};

}  // namespace ldw

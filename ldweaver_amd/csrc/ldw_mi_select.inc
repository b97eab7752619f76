// Part of ldw_mi.hip (inside namespace ldw): the long-range selection — histogram pick (R/computePairwiseMI.R:352-354), the general path
// (gather, two radix sorts) and the sort-free path (radix select of the threshold, bitmap ranks), per block and per span segment.
// ------------------------------------------------------------------------------------------------
// long-range selection
// ------------------------------------------------------------------------------------------------
struct PickOut {
    long long n;        // number of long-range pairs in the block
    long long lo, hi;   // 1-based ranks of the two order statistics of quantile type 7
    long long n_below;  // pairs in buckets below B
    double index, prob;
    int B;              // first bucket gathered
    int spec_ok;        // the speculative candidate list of the epilogue covers bucket B
    int B_true, over;   // bucket that holds rank lo (before the speculative override); over: bit 0 a pair list overflowed, bit 1 the maybe list did
    unsigned long long n_cand;  // filled by k_lr_gather
    long long n_kept;           // filled by k_lr_thresh
    double disc_thresh;
    long long kstart;
    long long n_below_true;     // pairs in buckets below B_true
};

// prob and quantile ranks of R/computePairwiseMI.R:352-354 (stats::quantile type 7), then the bucket
// holding rank lo.  One workgroup: chunked prefix sum over the NBINS counters.
// In speculative mode (spec_B >= 0) the histogram only holds buckets >= spec_B; n_total is the block's long-range
// pair count known to the host, and everything below spec_B is lumped into one virtual bucket.
__device__ __forceinline__ void pick_bucket_body(const unsigned long long *__restrict__ hist, double lr_retain, double lr_approx, int spec_B,
                                                 long long n_total, PickOut *__restrict__ out, const unsigned int *__restrict__ pl_n,
                                                 unsigned int pl_cap) {
    __shared__ long long part[256];
    __shared__ long long s_lo;
    constexpr int PER = NBINS / 256;
    const int t = threadIdx.x;
    long long loc[PER], sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        loc[k] = (long long)hist[t * PER + k];
        sum += loc[k];
    }
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        long long above = 0;
        for (int i = 0; i < 256; ++i) above += part[i];
        // speculative mode: pairs below spec_B were not histogrammed
        long long run = spec_B >= 0 ? n_total - above : 0;
        for (int i = 0; i < 256; ++i) {
            const long long v = part[i];
            part[i] = run;
            run += v;
        }
        PickOut o;
        memset(&o, 0, sizeof(o));
        o.n_cand = out->n_cand;  // speculative candidates appended by the epilogue
        o.n = run;
        o.B = NBINS;
        o.B_true = NBINS;
        o.disc_thresh = nan("");
        if (run > 0) {
            const double dn = (double)run;
            // every operation rounded on its own, in the reference's order (ldw_dev.h: lr_prob, q7_index)
            double prob = lr_prob(lr_retain, dn, lr_approx);
            if (!(prob > 0.0)) prob = 0.0;
            o.prob = prob;
            o.index = q7_index(dn - 1.0, prob);
            o.lo = (long long)floor(o.index);
            o.hi = (long long)ceil(o.index);
        }
        *out = o;
        s_lo = o.lo;
    }
    __syncthreads();
    const long long lo = s_lo;
    if (lo <= 0) return;
    long long cum = part[t];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (cum < lo && cum + loc[k] >= lo) {  // exactly one (thread, k) satisfies this
            out->B = t * PER + k;
            out->B_true = t * PER + k;
            out->n_below = cum;
            out->n_below_true = cum;
        }
        cum += loc[k];
    }
    __syncthreads();
    if (spec_B < 0) return;
    // speculative list = every long-range pair with bucket >= spec_B: usable iff rank lo lies at or above spec_B,
    // i.e. iff some bucket >= spec_B was found to hold it (the unhistogrammed mass below spec_B precedes part[0])
    if (lo > part[0]) {
        cum = part[t];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (t * PER + k == spec_B) {
                out->B = spec_B;
                out->n_below = cum;
                // a pair list of the approximate path that overflowed lost candidates: treat like a guess that was too high
                int over = 0;
                if (pl_n) {
                    for (int i = 0; i < PAIR_PATHS * PAIR_SHARDS; ++i) over |= pl_n[i] > pl_cap ? 1 : 0;
                    over |= pl_n[PH_MAYBE_OVER] > pl_cap ? 2 : 0;   // (the maybe list's overflow, k_screen_maybe)
                }
                out->over = over;
                out->spec_ok = over ? 0 : 1;
            }
            cum += loc[k];
        }
    } else if (t == 0) {
        out->n_cand = 0;  // guess too high: the fallback gather starts from an empty list
    }
}

__global__ __launch_bounds__(256) void k_pick_bucket(const unsigned long long *__restrict__ hist, double lr_retain,
                                                     double lr_approx, int spec_B, long long n_total,
                                                     PickOut *__restrict__ out, const unsigned int *__restrict__ pl_n, unsigned int pl_cap) {
    pick_bucket_body(hist, lr_retain, lr_approx, spec_B, n_total, out, pl_n, pl_cap);
}

// the same for every reference block of a span at once (blockIdx.x = segment): its own histogram, long-range pair count and pick
// record; the pair lists (and their overflow test) are the span's
struct PickSpanArgs {
    long long n_total[LDW_SPAN_MAX];
};
__global__ __launch_bounds__(256) void k_pick_bucket_span(const unsigned long long *__restrict__ hist, double lr_retain, double lr_approx, int spec_B,
                                                          PickSpanArgs S, char *__restrict__ picks, size_t pick_stride,
                                                          const unsigned int *__restrict__ pl_n, unsigned int pl_cap) {
    const int k = (int)blockIdx.x;
    pick_bucket_body(hist + (size_t)k * NBINS, lr_retain, lr_approx, spec_B, S.n_total[k], reinterpret_cast<PickOut *>(picks + (size_t)k * pick_stride), pl_n,
                     pl_cap);
}

struct GatherArgs {
    const double *MI;
    const ColInfo *cols;
    int nf, nt, lower_only;
};

// gather every long-range pair whose bucket is >= B: (MI key, order key)
__global__ __launch_bounds__(256) void k_lr_gather(GatherArgs S, PickOut *__restrict__ pick, uint64_t *__restrict__ ckey,
                                                   uint64_t *__restrict__ cval) {
    const int B = pick->B;
    if (B >= NBINS) return;
    const double lo_val = B > 0 ? bucket_lo(B) : 0.0;
    const int b0 = blockIdx.x * 16;
    for (int bb = 0; bb < 16; ++bb) {
        const int b_loc = b0 + bb;
        if (b_loc >= S.nt) break;
        const ColInfo c = S.cols[b_loc];
        const double *col = S.MI + (int64_t)b_loc * S.nf;
        for (int a_loc = threadIdx.x; a_loc < S.nf; a_loc += 256) {
            const int seg = pair_seg(a_loc, b_loc, S.lower_only);
            if (seg < 0) continue;  // also skips the never-written part of a diagonal block
            const double mi = col[a_loc];
            if (B > 0 && mi < lo_val) continue;  // cheap reject; the bucket test below decides
            if (col_is_sr(c, a_loc)) continue;
            if (mi_bucket(mi) < B) continue;
            const unsigned long long p = atomicAdd(&pick->n_cand, 1ull);
            ckey[p] = f64_key(mi);
            cval[p] = ((uint64_t)seg << 62) | ((uint64_t)a_loc + (uint64_t)b_loc * (uint64_t)S.nf);
        }
    }
}

// the same gather for a block in generic order (k_gen_count / k_gen_emit_sr above): the predicate instead of the intervals
__global__ __launch_bounds__(256) void k_gen_gather(GenArgs S, PickOut *__restrict__ pick, uint64_t *__restrict__ ckey, uint64_t *__restrict__ cval) {
    const int B = pick->B;
    if (B >= NBINS) return;
    const int lane = threadIdx.x & 63, b_loc = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b_loc >= S.nt) return;
    const double pos1 = (double)S.POS[S.idx_t[b_loc]];
    const double *col = S.MI + (int64_t)b_loc * S.nf;
    for (int a_loc = lane; a_loc < S.nf; a_loc += 64) {
        const int seg = pair_seg(a_loc, b_loc, S.lower_only);
        if (seg < 0) continue;
        const double mi = col[a_loc];
        if (mi_bucket(mi) < B) continue;
        if (gen_is_sr(S, a_loc, pos1)) continue;
        const unsigned long long p = atomicAdd(&pick->n_cand, 1ull);
        ckey[p] = f64_key(mi);
        cval[p] = ((uint64_t)seg << 62) | ((uint64_t)a_loc + (uint64_t)b_loc * (uint64_t)S.nf);
    }
}


// candidates sorted ascending by MI: quantile type 7, then first kept index
__global__ void k_lr_thresh(const uint64_t *__restrict__ skey, PickOut *__restrict__ pick) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    PickOut o = *pick;
    const long long m = (long long)o.n_cand;
    if (o.n <= 0 || m <= 0) {
        pick->n_kept = 0;
        pick->kstart = 0;
        return;
    }
    const long long off = o.n - m;  // ranks below the candidate set
    const double xlo = key_f64(skey[o.lo - off - 1]);
    const double xhi = key_f64(skey[o.hi - off - 1]);
    double qs = xlo;
    if (o.index > (double)o.lo && xhi != qs) {
        const double h = o.index - (double)o.lo;
        qs = q7_interp(h, qs, xhi);   // (no fma: ldw_dev.h)
    }
    const uint64_t kq = f64_key(qs);
    long long lo = 0, hi = m;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (skey[mid] < kq) lo = mid + 1; else hi = mid;
    }
    pick->disc_thresh = qs;
    pick->kstart = lo;
    pick->n_kept = m - lo;
}

// kept candidates keep their order key, the rest sink to the end of the second sort
__global__ void k_lr_mark(const uint64_t *__restrict__ skey, const uint64_t *__restrict__ sval,
                          const PickOut *__restrict__ pick, uint64_t *__restrict__ okey, uint64_t *__restrict__ oval,
                          long long m) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= m) return;
    const bool keep = i >= pick->kstart;
    okey[i] = keep ? sval[i] : ~0ull;
    oval[i] = skey[i];
}

__global__ void k_lr_append(const uint64_t *__restrict__ okey, const uint64_t *__restrict__ oval,
                            const PickOut *__restrict__ pick, const int32_t *__restrict__ idx_f,
                            const int32_t *__restrict__ idx_t, int nf, const int64_t *__restrict__ lr_count,
                            int32_t *__restrict__ out_a, int32_t *__restrict__ out_b, double *__restrict__ out_mi) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= pick->n_kept) return;
    const uint64_t c = okey[i] & 0x3FFFFFFFFFFFFFFFull;
    const int a_loc = (int)(c % (uint64_t)nf), b_loc = (int)(c / (uint64_t)nf);
    const int64_t dst = *lr_count + i;
    out_a[dst] = idx_f[a_loc];
    out_b[dst] = idx_t[b_loc];
    out_mi[dst] = key_f64(oval[i]);
}

// ------------------------------------------------------------------------------------------------
// Selection without a sort (the common case: <= 32768 candidates above the guessed bucket), four small launches:
//   k_sel_thresh  ONE workgroup, every thread keeps 32 MI keys in registers.  The two order statistics of quantile type 7 by an
//                 11-bit-digit RADIX SELECT (6 passes, an LDS histogram each; a wave first folds the lanes that share its first
//                 lane's bin into one LDS atomic, because the top digits of the candidates nearly all coincide), the smallest key
//                 above for x[hi], the threshold with R's own rule.
//   k_sel_mark    one thread per candidate: every kept candidate sets its bit in a BITMAP over the block's row-order key space
//                 (bit = segment * nf * nt + a + b * nf) and counts itself in its 1024-bit chunk and its 65536-bit super-chunk.
//   k_sel_scatter one thread per candidate: rank = (super-chunks before, scanned per workgroup in LDS) + (chunks before, in the
//                 super-chunk) + (bits before, in the chunk) = the row's position in the reference's row order
//                 (R/computePairwiseMI.R:306-331: upper rows column-major, then lower) -> written straight to its final place.
//   k_sel_clear   zeroes the bitmap words and counters that were touched (all three arrays stay all-zero between blocks).
// Same results as the two radix sorts of the general path, which stays for blocks without a bucket guess, speculation misses,
// more candidates and key spaces beyond 2^32 bits.
// ------------------------------------------------------------------------------------------------
constexpr int SEL_CHUNK_BITS = 1024, SEL_CHUNK_WORDS = SEL_CHUNK_BITS / 32, SEL_SUPER = 64;   // super-chunk = 64 chunks
constexpr int SEL_DIGIT = 11, SEL_BINS = 1 << SEL_DIGIT;
constexpr int SEL_MAX = 1 << 20;          // candidates the sort-free path takes
constexpr int SEL_MAX_SUPER = 8192;       // super-chunks a scatter workgroup can scan in LDS: key spaces up to 2^29 bits

__device__ __forceinline__ uint64_t sel_order_key(uint64_t cv, uint64_t space) {   // cv = seg << 62 | (a + b * nf)
    return (cv >> 62) * space + (cv & 0x3FFFFFFFFFFFFFFFull);
}

constexpr int SEL_LIST = 6144;   // keys of the threshold's bucket a k_sel_thresh workgroup keeps in LDS (more: it re-reads the global list)

__device__ __forceinline__ void sel_thresh_body(const uint64_t *__restrict__ ckey, PickOut *__restrict__ pick) {
    __shared__ uint64_t list[SEL_LIST];
    __shared__ unsigned int hist[SEL_BINS];
    __shared__ unsigned int wsum[16];
    __shared__ unsigned int s_n;
    __shared__ unsigned long long s_prefix, s_min, s_above;
    __shared__ long long s_k, s_less, s_eq;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const PickOut o = *pick;
    const long long m = (long long)o.n_cand;
    if (o.n <= 0 || m <= 0 || o.B_true >= NBINS) {
        if (t == 0) {
            pick->n_kept = 0;
            pick->kstart = -1;     // (as a key: above every candidate)
        }
        return;
    }
    // Phase A: the keys of the bucket that holds rank lo (the histogram that found it counts with the same mi_bucket) go to the
    // LDS list; the smallest key of the buckets above is x[hi] when rank hi leaves the bucket.  8 loads in flight per thread.
    if (t == 0) {
        s_n = 0u;
        s_above = ~0ull;
        s_prefix = 0ull;
        s_k = o.lo - o.n_below_true - 1;     // 0-based rank of x[lo] inside its bucket
        s_less = 0;
        s_eq = 0;
    }
    __syncthreads();
    unsigned long long above = ~0ull;
    for (long long base = 0; base < m; base += 8 * 1024) {
        uint64_t k8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long long i = base + (long long)j * 1024 + t;
            k8[j] = i < m ? ckey[i] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long long i = base + (long long)j * 1024 + t;
            const int bk = i < m ? mi_bucket(key_f64(k8[j])) : -1;
            if (bk > o.B_true && k8[j] < above) above = k8[j];
            const bool in = bk == o.B_true;
            const unsigned long long mk = __ballot(in);
            if (mk == 0ull) continue;
            unsigned int pos = 0;
            if (lane == __builtin_ctzll(mk)) pos = atomicAdd(&s_n, (unsigned int)__popcll(mk));
            pos = (unsigned int)__shfl((int)pos, __builtin_ctzll(mk)) + (unsigned int)__popcll(mk & ((1ull << lane) - 1ull));
            if (in && pos < SEL_LIST) list[pos] = k8[j];
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long y = __shfl_xor(above, d);
        above = y < above ? y : above;
    }
    if (lane == 0) atomicMin(&s_above, above);
    __syncthreads();
    const unsigned int n_in = s_n;
    const bool in_lds = n_in <= SEL_LIST;
    // visit every key of the bucket: the LDS list, or (huge tie groups) the global list once more
    auto n_items = [&]() -> long long { return in_lds ? (long long)n_in : m; };
    auto item = [&](long long i, uint64_t &k) -> bool {
        if (in_lds) {
            k = list[i];
            return true;
        }
        k = ckey[i];
        return mi_bucket(key_f64(k)) == o.B_true;
    };
    // Phase B: radix select of rank s_k among them, 11-bit digits from the top
    uint64_t mask = 0ull;
    const long long n_it = n_items();
    for (int pass = 0; pass < 6; ++pass) {
        const int shift = pass < 5 ? 64 - SEL_DIGIT * (pass + 1) : 0;     // 53, 42, 31, 20, 9, then the last 9 bits
        const unsigned int dmask = pass < 5 ? (unsigned int)SEL_BINS - 1u : 511u;
        for (int i = t; i < SEL_BINS; i += 1024) hist[i] = 0u;
        __syncthreads();
        const uint64_t prefix = s_prefix;
        for (long long i0 = 0; i0 < n_it; i0 += 1024) {
            const long long i = i0 + t;
            uint64_t k = 0ull;
            const bool in = i < n_it && item(i, k) && (k & mask) == prefix;
            const unsigned int bin = (unsigned int)(k >> shift) & dmask;
            const unsigned long long act = __ballot(in);
            if (act == 0ull) continue;
            const unsigned int b0 = (unsigned int)__shfl((int)bin, __builtin_ctzll(act));
            const unsigned long long same = __ballot(in && bin == b0);      // the top digits nearly all coincide: one atomic for them
            if (in && bin == b0) {
                if (lane == __builtin_ctzll(same)) atomicAdd(&hist[b0], (unsigned int)__popcll(same));
            } else if (in) {
                atomicAdd(&hist[bin], 1u);
            }
        }
        __syncthreads();
        // the bin that holds rank s_k: every thread owns two adjacent bins
        const unsigned int h0 = hist[2 * t], h1 = hist[2 * t + 1];
        unsigned int x = h0 + h1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        unsigned int base = 0;
        for (int w = 0; w < wave; ++w) base += wsum[w];
        const long long incl = (long long)base + x, excl = incl - (h0 + h1), k = s_k;
        __syncthreads();
        if (k >= excl && k < incl) {        // exactly one thread
            const int b = (k < excl + h0) ? 0 : 1;
            const long long before = excl + (b ? h0 : 0);
            s_prefix = prefix | ((uint64_t)(2 * t + b) << shift);
            s_k = k - before;
            s_less += before;
            s_eq = b ? h1 : h0;
        }
        __syncthreads();
        mask |= (uint64_t)dmask << shift;
    }
    const uint64_t v_lo = s_prefix;                  // key of rank lo; s_less keys of the bucket are smaller, s_eq equal
    uint64_t v_hi = v_lo;
    const long long r_in = o.lo - o.n_below_true - 1;
    if (o.hi > o.lo && r_in + 1 >= s_less + s_eq) {  // x[hi] is the smallest key above v_lo: in the bucket, or the first one above it
        if (t == 0) s_min = s_above;
        __syncthreads();
        unsigned long long mn = ~0ull;
        for (long long i0 = 0; i0 < n_it; i0 += 1024) {
            const long long i = i0 + t;
            uint64_t k = 0ull;
            if (i < n_it && item(i, k) && k > v_lo && k < mn) mn = k;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned long long y = __shfl_xor(mn, d);
            mn = y < mn ? y : mn;
        }
        if (lane == 0) atomicMin(&s_min, mn);
        __syncthreads();
        v_hi = s_min;
    }
    if (t == 0) {
        const double xlo = key_f64(v_lo), xhi = key_f64(v_hi);
        double qs = xlo;
        if (o.index > (double)o.lo && xhi != qs) {   // stats::quantile type 7 (the interpolation is skipped on a tie)
            const double h = o.index - (double)o.lo;
            qs = q7_interp(h, qs, xhi);   // (no fma: ldw_dev.h)
        }
        pick->disc_thresh = qs;
        pick->n_kept = 0;                            // counted by k_sel_mark
        pick->kstart = (long long)f64_key(qs);       // (reused: the threshold key, read by the kernels below)
    }
}

__global__ __launch_bounds__(1024) void k_sel_thresh(const uint64_t *__restrict__ ckey, PickOut *__restrict__ pick) { sel_thresh_body(ckey, pick); }

// The selection of all reference blocks of a span in ONE launch per stage (blockIdx.y = segment): each segment has its own candidate
// list, pick record, bitmap and counters; the rows of segment k go behind those of segments 0 .. k-1 (their n_kept are final when the
// scatter starts), which is the order the reference appends in.
struct SelSpan {
    int n;
    const uint64_t *ck[LDW_SPAN_MAX], *cv[LDW_SPAN_MAX];
    PickOut *pick[LDW_SPAN_MAX];
    const int32_t *idx_t[LDW_SPAN_MAX];
    uint64_t space[LDW_SPAN_MAX];
    uint32_t *bitmap[LDW_SPAN_MAX], *chunks[LDW_SPAN_MAX], *supers[LDW_SPAN_MAX];
    int n_super[LDW_SPAN_MAX];
};
__global__ __launch_bounds__(1024) void k_sel_thresh_span(SelSpan S) { sel_thresh_body(S.ck[blockIdx.y], S.pick[blockIdx.y]); }

__device__ __forceinline__ void sel_mark_body(const uint64_t *__restrict__ ckey, const uint64_t *__restrict__ cval, PickOut *__restrict__ pick,
                                              uint64_t space, uint32_t *__restrict__ bitmap, uint32_t *__restrict__ chunk_cnt,
                                              uint32_t *__restrict__ super_cnt) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    const bool keep = i < (long long)pick->n_cand && ckey[i] >= (uint64_t)pick->kstart;
    if (keep) {
        const uint64_t ok = sel_order_key(cval[i], space);
        atomicOr(&bitmap[ok >> 5], 1u << (ok & 31));
        atomicAdd(&chunk_cnt[ok / SEL_CHUNK_BITS], 1u);
        atomicAdd(&super_cnt[ok / (SEL_CHUNK_BITS * SEL_SUPER)], 1u);
    }
    const unsigned long long mk = __ballot(keep);
    if (mk != 0ull && (threadIdx.x & 63) == __builtin_ctzll(mk)) atomicAdd((unsigned long long *)&pick->n_kept, (unsigned long long)__popcll(mk));
}

__global__ __launch_bounds__(256) void k_sel_mark(const uint64_t *__restrict__ ckey, const uint64_t *__restrict__ cval, PickOut *__restrict__ pick,
                                                  uint64_t space, uint32_t *__restrict__ bitmap, uint32_t *__restrict__ chunk_cnt,
                                                  uint32_t *__restrict__ super_cnt) {
    sel_mark_body(ckey, cval, pick, space, bitmap, chunk_cnt, super_cnt);
}
__global__ __launch_bounds__(256) void k_sel_mark_span(SelSpan S) {
    const int y = blockIdx.y;
    sel_mark_body(S.ck[y], S.cv[y], S.pick[y], S.space[y], S.bitmap[y], S.chunks[y], S.supers[y]);
}

__device__ __forceinline__ void sel_scatter_body(const uint64_t *__restrict__ ckey, const uint64_t *__restrict__ cval, const PickOut *__restrict__ pick,
                                                 uint64_t space, const uint32_t *__restrict__ bitmap, const uint32_t *__restrict__ chunk_cnt,
                                                 const uint32_t *__restrict__ super_cnt, int n_super, const int32_t *__restrict__ idx_f,
                                                 const int32_t *__restrict__ idx_t, int nf, int64_t row_base,
                                                 int32_t *__restrict__ out_a, int32_t *__restrict__ out_b, double *__restrict__ out_mi) {
    __shared__ unsigned int spre[SEL_MAX_SUPER];
    __shared__ unsigned int wtot[4];
    // exclusive scan of the super-chunk counters, per workgroup: strips of consecutive counters per thread
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = (n_super + 255) / 256, s0 = t * per, s1 = s0 + per < n_super ? s0 + per : n_super;
    unsigned int sum = 0;
    for (int q = s0; q < s1; ++q) sum += super_cnt[q];
    unsigned int x = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) wtot[wave] = x;
    __syncthreads();
    unsigned int run = x - sum;
    for (int w = 0; w < wave; ++w) run += wtot[w];
    for (int q = s0; q < s1; ++q) {
        spre[q] = run;
        run += super_cnt[q];
    }
    __syncthreads();
    const long long i = blockIdx.x * (long long)blockDim.x + t;
    if (i >= (long long)pick->n_cand) return;
    const uint64_t k = ckey[i];
    if (k < (uint64_t)pick->kstart) return;
    const uint64_t cv = cval[i], ok = sel_order_key(cv, space);
    const uint64_t chunk = ok / SEL_CHUNK_BITS, sup = chunk / SEL_SUPER, w_end = ok >> 5;
    unsigned int rank = spre[sup];
    for (uint64_t q = sup * SEL_SUPER; q < chunk; ++q) rank += chunk_cnt[q];
    for (uint64_t w = chunk * SEL_CHUNK_WORDS; w < w_end; ++w) rank += __popc(bitmap[w]);
    rank += __popc(bitmap[w_end] & ((1u << (ok & 31)) - 1u));
    if ((long long)rank >= pick->n_kept) return;   // (cannot happen; never write past the rows reserved for this block)
    const uint64_t c = cv & 0x3FFFFFFFFFFFFFFFull;
    const int a_loc = (int)(c % (uint64_t)nf), b_loc = (int)(c / (uint64_t)nf);
    const int64_t dst = row_base + rank;
    out_a[dst] = idx_f[a_loc];
    out_b[dst] = idx_t[b_loc];
    out_mi[dst] = key_f64(k);
}
__global__ __launch_bounds__(256) void k_sel_scatter(const uint64_t *__restrict__ ckey, const uint64_t *__restrict__ cval, const PickOut *__restrict__ pick,
                                                     uint64_t space, const uint32_t *__restrict__ bitmap, const uint32_t *__restrict__ chunk_cnt,
                                                     const uint32_t *__restrict__ super_cnt, int n_super, const int32_t *__restrict__ idx_f,
                                                     const int32_t *__restrict__ idx_t, int nf, const int64_t *__restrict__ lr_count,
                                                     int32_t *__restrict__ out_a, int32_t *__restrict__ out_b, double *__restrict__ out_mi) {
    sel_scatter_body(ckey, cval, pick, space, bitmap, chunk_cnt, super_cnt, n_super, idx_f, idx_t, nf, *lr_count, out_a, out_b, out_mi);
}
__global__ __launch_bounds__(256) void k_sel_scatter_span(SelSpan S, const int32_t *__restrict__ idx_f, int nf, const int64_t *__restrict__ lr_count,
                                                          int32_t *__restrict__ out_a, int32_t *__restrict__ out_b, double *__restrict__ out_mi) {
    const int y = blockIdx.y;
    int64_t base = *lr_count;
    for (int j = 0; j < y; ++j) base += S.pick[j]->n_kept;   // (final: k_sel_mark_span of every segment has finished)
    sel_scatter_body(S.ck[y], S.cv[y], S.pick[y], S.space[y], S.bitmap[y], S.chunks[y], S.supers[y], S.n_super[y], idx_f, S.idx_t[y], nf, base, out_a, out_b,
                     out_mi);
}

__device__ __forceinline__ void sel_clear_body(const uint64_t *__restrict__ ckey, const uint64_t *__restrict__ cval, const PickOut *__restrict__ pick,
                                               uint64_t space, uint32_t *__restrict__ bitmap, uint32_t *__restrict__ chunk_cnt,
                                               uint32_t *__restrict__ super_cnt) {
    const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
    if (i >= (long long)pick->n_cand) return;
    if (ckey[i] < (uint64_t)pick->kstart) return;
    const uint64_t ok = sel_order_key(cval[i], space);
    bitmap[ok >> 5] = 0u;
    chunk_cnt[ok / SEL_CHUNK_BITS] = 0u;
    super_cnt[ok / (SEL_CHUNK_BITS * SEL_SUPER)] = 0u;
}

__global__ __launch_bounds__(256) void k_sel_clear(const uint64_t *__restrict__ ckey, const uint64_t *__restrict__ cval, const PickOut *__restrict__ pick,
                                                   uint64_t space, uint32_t *__restrict__ bitmap, uint32_t *__restrict__ chunk_cnt,
                                                   uint32_t *__restrict__ super_cnt) {
    sel_clear_body(ckey, cval, pick, space, bitmap, chunk_cnt, super_cnt);
}
__global__ __launch_bounds__(256) void k_sel_clear_span(SelSpan S) {
    const int y = blockIdx.y;
    sel_clear_body(S.ck[y], S.cv[y], S.pick[y], S.space[y], S.bitmap[y], S.chunks[y], S.supers[y]);
}
// running count and stats of every reference block of a span (one thread)
struct SpanDoneArgs {
    long long n_sr[LDW_SPAN_MAX];
};
__global__ void k_span_done(SelSpan S, SpanDoneArgs D, int64_t *lr_count, int64_t *stats_i, double *stats_d) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int k = 0; k < S.n; ++k) {
        const PickOut *pk = S.pick[k];
        *lr_count += pk->n_kept;
        stats_i[k * 3 + 0] = pk->n;
        stats_i[k * 3 + 1] = pk->n_kept;
        stats_i[k * 3 + 2] = D.n_sr[k];
        stats_d[k] = pk->disc_thresh;
    }
}

// (a, b) of the short-range rows of ONE block of contiguous SNP ranges, from positions alone: the rows a pass emits there are a pure
// function of POS, g, sr_dist and the block geometry (R/computePairwiseMI.R:306-333) — what lets a multi-GPU gather send only the MI column of
// the short-range table (8 of 16 bytes per row) and rank 0 rebuild the index columns itself.  One wave per to-side SNP.
__global__ __launch_bounds__(256) void k_sr_fill(const ColInfo *__restrict__ cols, int nf, int nt, int fs0, int ts0, int lower_only, int64_t base,
                                                 int32_t *__restrict__ a_out, int32_t *__restrict__ b_out) {
    const int lane = threadIdx.x & 63, b_loc = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b_loc >= nt) return;
    const ColInfo c = cols[b_loc];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int a_loc = c.s[k] + lane; a_loc < c.e[k]; a_loc += 64) {
            const int seg = pair_seg(a_loc, b_loc, lower_only);
            if (seg < 0) continue;
            const int64_t dst = base + (seg == 0 ? c.off_u + col_count(c, 0, a_loc) : c.off_l + col_count(c, b_loc + 1, a_loc));
            a_out[dst] = fs0 + a_loc;
            b_out[dst] = ts0 + b_loc;
        }
}

// ---- r05: the same index columns with the intervals built ON THE DEVICE (ldw_sr_pairs_fill: contiguous blocks of an alignment whose POS ascends).  The host
// loop of build_cols is 85 ns per column — 17 ms for the 20 band blocks of C4, every step of a multi-GPU job's rank 0 — for five binary searches per column.
struct SrBlkDev {
    int32_t fs0, nf, ts0, nt, diag, pad;
    int64_t col0;   // first column of this block in the concatenated column arrays
};

__device__ __forceinline__ int64_t lb_pos(const int32_t *__restrict__ P, int64_t n, double v) {   // first a with P[a] >= v
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((double)P[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int64_t ub_pos(const int32_t *__restrict__ P, int64_t n, double v) {   // first a with P[a] > v
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (!(v < (double)P[mid])) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One thread per (block, column): build_cols' candidate windows, merge and boundary checks with the reference's predicate; a column whose check fails sets
// *bad (the caller then takes the host path, which rebuilds such a column by scanning).
__global__ __launch_bounds__(256) void k_cols_dev(const int32_t *__restrict__ POS, double g, double sr_dist, const SrBlkDev *__restrict__ blk, int nblk,
                                                  int64_t ncols, ColInfo *__restrict__ cols, int32_t *__restrict__ cu, int32_t *__restrict__ cl,
                                                  int *__restrict__ bad) {
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= ncols) return;
    int lo = 0, hi = nblk;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk[mid].col0 <= col) lo = mid;
        else hi = mid;
    }
    const SrBlkDev B = blk[lo];
    const int64_t b = col - B.col0, nf = B.nf;
    const int32_t *__restrict__ pf = POS + B.fs0;
    const double p1 = (double)POS[B.ts0 + b];
    auto Pr = [&](int64_t a) { return circ_len(p1, (double)pf[a], g) <= sr_dist; };
    int64_t iv[3][2];
    iv[0][0] = 0;
    iv[0][1] = ub_pos(pf, nf, p1 + sr_dist - g);
    iv[1][0] = lb_pos(pf, nf, p1 - sr_dist);
    iv[1][1] = ub_pos(pf, nf, p1 + sr_dist);
    iv[2][0] = lb_pos(pf, nf, p1 - sr_dist + g);
    iv[2][1] = nf;
    int n = 0;
    int64_t m[3][2] = {{0, 0}, {0, 0}, {0, 0}};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (iv[k][1] <= iv[k][0]) continue;
        if (n > 0 && iv[k][0] <= m[n - 1][1]) m[n - 1][1] = m[n - 1][1] > iv[k][1] ? m[n - 1][1] : iv[k][1];
        else {
            m[n][0] = iv[k][0];
            m[n][1] = iv[k][1];
            ++n;
        }
    }
    bool ok = true;
    for (int k = 0; k < n && ok; ++k) {
        ok = Pr(m[k][0]) && Pr(m[k][1] - 1);
        if (ok && m[k][0] > 0) ok = !Pr(m[k][0] - 1);
        if (ok && m[k][1] < nf) ok = !Pr(m[k][1]);
    }
    if (n == 0 && nf > 0) ok = !Pr(0) && !Pr(nf - 1);
    if (!ok) atomicOr(bad, 1);
    ColInfo ci;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ci.s[k] = k < n ? (int32_t)m[k][0] : 0;
        ci.e[k] = k < n ? (int32_t)m[k][1] : 0;
    }
    ci.pad[0] = ci.pad[1] = 0;
    ci.off_u = ci.off_l = 0;
    cu[col] = B.diag ? 0 : col_count(ci, 0, (int)(b < nf ? b : nf));
    cl[col] = col_count(ci, (int)(b + 1 < nf ? b + 1 : nf), (int)nf);
    cols[col] = ci;
}

// One workgroup per block: the row offsets of its columns — all upper-segment columns, then all lower-segment ones (R/computePairwiseMI.R:306-310) — and
// the block's row count.
__global__ __launch_bounds__(256) void k_cols_scan(const SrBlkDev *__restrict__ blk, ColInfo *__restrict__ cols, const int32_t *__restrict__ cu,
                                                   const int32_t *__restrict__ cl, int64_t *__restrict__ rows) {
    __shared__ long long wsum[4], carry;
    const SrBlkDev B = blk[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    long long total_u = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const int32_t *__restrict__ cnt = pass == 0 ? cu : cl;
        if (tid == 0) carry = pass == 0 ? 0 : total_u;
        __syncthreads();
        for (int64_t b0 = 0; b0 < B.nt; b0 += 256) {
            const int64_t b = b0 + tid;
            const long long v = b < B.nt ? (long long)cnt[B.col0 + b] : 0;
            long long incl = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const long long t = __shfl_up(incl, o);
                if (lane >= o) incl += t;
            }
            if (lane == 63) wsum[wv] = incl;
            __syncthreads();
            long long before = carry;
            for (int w = 0; w < wv; ++w) before += wsum[w];
            if (b < B.nt) {
                if (pass == 0) cols[B.col0 + b].off_u = before + incl - v;
                else cols[B.col0 + b].off_l = before + incl - v;
            }
            __syncthreads();
            if (tid == 0) carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
            __syncthreads();
        }
        if (pass == 0) total_u = carry;
    }
    if (tid == 0) rows[blockIdx.x] = carry;   // upper + lower rows
}

// base[k] = rows of the blocks before k; base[nblk] = all rows
__global__ void k_blk_bases(const int64_t *__restrict__ rows, int nblk, int64_t *__restrict__ base) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t run = 0;
    for (int k = 0; k < nblk; ++k) {
        base[k] = run;
        run += rows[k];
    }
    base[nblk] = run;
}

// k_sr_fill over all blocks at once: one wave per column
__global__ __launch_bounds__(256) void k_sr_fill_all(const ColInfo *__restrict__ cols, const SrBlkDev *__restrict__ blk, int nblk, int64_t ncols,
                                                     const int64_t *__restrict__ base, int32_t *__restrict__ a_out, int32_t *__restrict__ b_out) {
    const int lane = threadIdx.x & 63;
    const int64_t col = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= ncols) return;
    int lo = 0, hi = nblk;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk[mid].col0 <= col) lo = mid;
        else hi = mid;
    }
    const SrBlkDev B = blk[lo];
    const int b_loc = (int)(col - B.col0);
    const ColInfo c = cols[col];
    const int64_t bs = base[lo];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        for (int a_loc = c.s[k] + lane; a_loc < c.e[k]; a_loc += 64) {
            const int seg = pair_seg(a_loc, b_loc, B.diag);
            if (seg < 0) continue;
            const int64_t dst = bs + (seg == 0 ? c.off_u + col_count(c, 0, a_loc) : c.off_l + col_count(c, b_loc + 1, a_loc));
            a_out[dst] = B.fs0 + a_loc;
            b_out[dst] = B.ts0 + b_loc;
        }
}

// running device-side counters and per-block stats
__global__ void k_block_done(PickOut *pick, int64_t *lr_count, int64_t n_sr_blk, int64_t *stats_i, double *stats_d) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    *lr_count += pick->n_kept;
    stats_i[0] = pick->n;
    stats_i[1] = pick->n_kept;
    stats_i[2] = n_sr_blk;
    stats_d[0] = pick->disc_thresh;
}


// Context, residency, set-up kernels and the small element-wise twins of libldweaver_amd.so.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <thread>
#include "ldw_internal.h"
#include "ldw_dev.h"
#include "ldw_fasta.h"
#include "ldw_links_read.h"
#include "ldw_slots.h"

namespace ldw {
int check_gpu(ldw_ctx *ctx) {
    LDW_REQUIRE(ctx != nullptr, LDW_ERR_ARG, "null context");
    LDW_HIP(hipSetDevice(ctx->device));
    return LDW_OK;
}
}  // namespace ldw

using namespace ldw;

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
namespace ldw {

// states [L][N] (tight) -> padded [L][Npad], pad value 255 (matches no state)
__global__ void k_pad_states(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int64_t L, int64_t N,
                             int64_t Npad) {
    const int64_t a = blockIdx.x;
    for (int64_t s = threadIdx.x; s < Npad; s += blockDim.x)
        dst[a * Npad + s] = s < N ? src[a * N + s] : (uint8_t)255;
}

__global__ void k_unpad_states(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int64_t L, int64_t N,
                               int64_t Npad) {
    const int64_t a = blockIdx.x;
    for (int64_t s = threadIdx.x; s < N; s += blockDim.x)
        dst[a * N + s] = src[a * Npad + s];
}

// 5-state encoder (src/getACGTNsites.cpp:229-265, encode_char in ldw_dev.h): chars [N][L_total] -> states [n_pos][Npad]
__global__ void k_encode(const char *__restrict__ chars, int64_t N, int64_t L_total, const int32_t *__restrict__ pos,
                         int64_t n_pos, uint8_t *__restrict__ states, int64_t Npad) {
    // tile transpose through LDS: 64 positions x 64 sequences per workgroup, coalesced on both sides
    // when the retained columns are dense; gathers when they are sparse.
    __shared__ uint8_t tile[64][65];
    const int64_t p0 = (int64_t)blockIdx.x * 64, s0 = (int64_t)blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;  // 256 threads: 64 x 4
    for (int i = ty; i < 64; i += 4) {                       // i: sequence within tile, tx: position
        const int64_t s = s0 + i, p = p0 + tx;
        uint8_t v = 255;
        if (s < N && p < n_pos) v = encode_char((unsigned char)chars[s * L_total + (pos[p] - 1)]);
        tile[i][tx] = v;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {  // i: position within tile, tx: sequence
        const int64_t p = p0 + i, s = s0 + tx;
        if (p < n_pos && s < Npad) states[p * Npad + s] = (s < N) ? tile[tx][i] : (uint8_t)255;
    }
}

// per-column allele counts of a raw alignment (src/getACGTNsites.cpp:58-70): one thread per column, coalesced along
// the sequence, five counters in registers
__global__ __launch_bounds__(256) void k_column_counts(const char *__restrict__ chars, int64_t N, int64_t L_total,
                                                       int32_t *__restrict__ counts) {
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= L_total) return;
    int c[5] = {0, 0, 0, 0, 0};
    for (int64_t s = 0; s < N; ++s) {
        const uint8_t st = encode_char((unsigned char)chars[s * L_total + j]);
#pragma unroll
        for (int x = 0; x < 5; ++x) c[x] += st == x;
    }
#pragma unroll
    for (int x = 0; x < 5; ++x) counts[j * 5 + x] = c[x];
}

// ---- the native FASTA feeder's kernels (host side: ldw_fasta.cpp) ----
// k_fasta_count_pack: one launch per chunk of rows [rows][Lp] (rows padded to Lp = L rounded up to 16 bytes by the reader).  A lane owns 16
// consecutive columns — one 16-byte load per row — for the whole launch, so the counts [Lp][5] are read, added to and written back without
// atomics (launches on one stream do not overlap).  A/C/G/T are counted, the fifth state is what is left.  With packed non-null the chunk's
// states also go out 4 bits each (8 bytes per lane and row), the device copy ldw_fasta_encode reads instead of the file.
constexpr int FA_COLS = 16;
__global__ __launch_bounds__(256) void k_fasta_count_pack(const uint8_t *__restrict__ chunk, int64_t rows, int64_t L, int64_t Lp,
                                                          int32_t *__restrict__ counts, uint8_t *__restrict__ packed) {
    const int64_t j0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * FA_COLS;
    if (j0 >= L) return;
    int c[FA_COLS][4] = {};
    for (int64_t r = 0; r < rows; ++r) {
        const uint4 v = *reinterpret_cast<const uint4 *>(chunk + r * Lp + j0);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint32_t pk[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < FA_COLS; ++k) {
            const uint32_t st = encode_char((unsigned char)(w[k >> 2] >> (8 * (k & 3))));
#pragma unroll
            for (int x = 0; x < 4; ++x) c[k][x] += st == (uint32_t)x;
            pk[k >> 3] |= st << (4 * (k & 7));
        }
        if (packed) *reinterpret_cast<uint2 *>(packed + r * (Lp / 2) + j0 / 2) = make_uint2(pk[0], pk[1]);
    }
    // the lane's 16 columns are 80 consecutive int32 of the counts (320 bytes, 64-byte aligned; the buffer is padded to Lp columns): 20
    // 16-byte read-modify-writes instead of 80 scattered dwords (a 1-row chunk of 2.2 M columns: 54 -> 36 us)
    int add[FA_COLS * 5];
#pragma unroll
    for (int k = 0; k < FA_COLS; ++k) {
#pragma unroll
        for (int x = 0; x < 4; ++x) add[k * 5 + x] = c[k][x];
        add[k * 5 + 4] = (int)rows - (c[k][0] + c[k][1] + c[k][2] + c[k][3]);
    }
    int4 *o = reinterpret_cast<int4 *>(counts + j0 * 5);
#pragma unroll
    for (int q = 0; q < FA_COLS * 5 / 4; ++q) {
        int4 v = o[q];
        v.x += add[4 * q];
        v.y += add[4 * q + 1];
        v.z += add[4 * q + 2];
        v.w += add[4 * q + 3];
        o[q] = v;
    }
}

// k_fasta_encode_rows: the retained columns of the sequences s0 .. s_end (one chunk of rows, or all of them from the packed copy) into
// states [n_pos][Npad], transposed through LDS in tiles of 64 positions x 64 sequences as k_encode; sequences from N on are the 255 padding
// (the launch of the last chunk runs to Npad, so the padding is written once).
template <bool Packed>
__global__ __launch_bounds__(256) void k_fasta_encode_rows(const uint8_t *__restrict__ src, int64_t stride, int64_t src_s0, int64_t s0,
                                                           int64_t s_end, int64_t N, const int32_t *__restrict__ pos, int64_t n_pos,
                                                           uint8_t *__restrict__ states, int64_t Npad) {
    __shared__ uint8_t tile[64][65];
    const int64_t p0 = (int64_t)blockIdx.x * 64, sb = s0 + (int64_t)blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t p = p0 + tx;
    const int64_t col = p < n_pos ? (int64_t)pos[p] - 1 : 0;
    for (int i = ty; i < 64; i += 4) {   // i: sequence within the tile, tx: position
        const int64_t s = sb + i;
        uint8_t v = 255;
        if (s < N && s < s_end && p < n_pos) {
            const uint8_t *row = src + (s - src_s0) * stride;
            v = Packed ? (uint8_t)((row[col >> 1] >> (4 * (col & 1))) & 15) : encode_char(row[col]);
        }
        tile[i][tx] = v;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {   // i: position within the tile, tx: sequence
        const int64_t q = p0 + i, s = sb + tx;
        if (q < n_pos && s < s_end) states[q * Npad + s] = tile[tx][i];
    }
}

// per-SNP state counts and fixed-point weighted marginals.  One wave per SNP; each lane reads 4
// consecutive sequences (one dword) per step.
__global__ __launch_bounds__(256) void k_counts_marginals(const uint8_t *__restrict__ states, int64_t L, int64_t Npad,
                                                          const int64_t *__restrict__ vfixed,  // may be null
                                                          int32_t *__restrict__ counts, int64_t *__restrict__ pfix) {
    const int lane = threadIdx.x & 63;
    const int64_t a = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= L) return;
    int cnt[5] = {0, 0, 0, 0, 0};
    long long pf[5] = {0, 0, 0, 0, 0};
    const uint32_t *row = reinterpret_cast<const uint32_t *>(states + a * Npad);
    for (int64_t q = lane; q < Npad / 4; q += 64) {
        const uint32_t w = row[q];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t st = (w >> (8 * k)) & 0xFF;
            const long long v = vfixed ? vfixed[q * 4 + k] : 0;
#pragma unroll
            for (int x = 0; x < 5; ++x) {
                const bool hit = st == (uint32_t)x;
                cnt[x] += hit ? 1 : 0;
                pf[x] += hit ? v : 0;
            }
        }
    }
#pragma unroll
    for (int x = 0; x < 5; ++x) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            cnt[x] += __shfl_xor(cnt[x], off);
            pf[x] += __shfl_xor(pf[x], off);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            counts[a * 5 + x] = cnt[x];
            if (pfix) pfix[a * 5 + x] = pf[x];
        }
    }
}

// .ACGTN2num (src/ACGTN2num_parallel.cpp:10-43): zero the reference-allele entry of each 5-column
__global__ void k_acgtn2num(double *__restrict__ nv, const char *__restrict__ ref, int64_t L) {
    const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (c >= L) return;
    const int rowi = acgtn_row(ref[c]);
    if (rowi >= 0) nv[c * 5 + rowi] = 0.0;
}

// .fastHadamard (src/computeMI.cpp:19), same association order
__global__ void k_fast_hadamard(double *__restrict__ MI, const double *__restrict__ den, const double *__restrict__ uq,
                                const double *__restrict__ pxy, const double *__restrict__ pxpy,
                                const double *__restrict__ RXY, const double *__restrict__ pXrX,
                                const double *__restrict__ pYrY, int64_t n) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
        const double d = ((pxpy[c] + RXY[c]) + pXrX[c]) + pYrY[c];
        MI[c] += ((uq[c] * pxy[c]) / den[c]) * log((pxy[c] / d) * den[c]);
    }
}

int launch_state_counts(ldw_ctx *c) {
    LDW_REQUIRE(ldw::have_alignment(c), LDW_ERR_STATE, "state counts: no alignment resident");
    if (int rc = c->rows.counts.reserve((size_t)c->L * 5 * 4)) return rc;
    hipLaunchKernelGGL(k_counts_marginals, dim3((unsigned)((c->L + 3) / 4)), dim3(256), 0, c->stream, c->states.as<uint8_t>(), c->L, c->Npad, (const int64_t *)nullptr,
                       c->rows.counts.as<int32_t>(), (int64_t *)nullptr);
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

int launch_fasta_count_pack(const uint8_t *chunk, int64_t rows, int64_t L, int64_t Lp, int32_t *counts, uint8_t *packed, hipStream_t s) {
    const int64_t lanes = (L + FA_COLS - 1) / FA_COLS;
    hipLaunchKernelGGL(k_fasta_count_pack, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, chunk, rows, L, Lp, counts, packed);
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

int launch_fasta_encode_rows(bool packed, const uint8_t *src, int64_t stride, int64_t src_s0, int64_t s0, int64_t s_end, int64_t N,
                             const int32_t *pos, int64_t n_pos, uint8_t *states, int64_t Npad, hipStream_t s) {
    const dim3 grid((unsigned)((n_pos + 63) / 64), (unsigned)((s_end - s0 + 63) / 64));
    if (packed)
        hipLaunchKernelGGL(k_fasta_encode_rows<true>, grid, dim3(256), 0, s, src, stride, src_s0, s0, s_end, N, pos, n_pos, states, Npad);
    else
        hipLaunchKernelGGL(k_fasta_encode_rows<false>, grid, dim3(256), 0, s, src, stride, src_s0, s0, s_end, N, pos, n_pos, states, Npad);
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

}  // namespace ldw

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int ldw_version(void) { return 100; }

int ldw_build_info(void) { return 0; }

int ldw_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int ldw_ctx_create(int device, ldw_ctx **out) {
    LDW_REQUIRE(out != nullptr, LDW_ERR_ARG, "ldw_ctx_create: out is null");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("ldw_ctx_create: no HIP device visible; this library has no CPU fallback");
        return LDW_ERR_NOGPU;
    }
    LDW_REQUIRE(device >= 0 && device < n, LDW_ERR_ARG, "ldw_ctx_create: device %d out of range (0..%d)", device, n - 1);
    LDW_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    LDW_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("ldw_ctx_create: device %d is %s; kernels are built for gfx950 only", device, prop.gcnArchName);
        return LDW_ERR_NOGPU;
    }
    // a half-built context is not handed out: every failing return below destroys it (and takes it off the live count); *out stays null, the error text is the failure's
    struct Destroy {
        void operator()(ldw_ctx *h) const {
            const std::string msg = ldw_last_error();
            ldw_ctx_destroy(h);
            ldw::set_error("%s", msg.c_str());
        }
    };
    std::unique_ptr<ldw_ctx, Destroy> guard(new ldw_ctx());
    ldw_ctx *c = guard.get();
    ldw::ctx_count(+1);
    c->device = device;
    c->n_cu = prop.multiProcessorCount;
    c->knobs.prune = getenv("LDW_NO_PRUNE") == nullptr;
    LDW_HIP(c->stream.ensure(hipStreamNonBlocking));
    for (auto &e : c->ev) LDW_HIP(e.ensure());
    // r04: the two extra streams of the all-pairs loop (hipStreamCreate: 12 ms each on this box), its events and pinned pick records are made
    // WITH the context, and the code objects of the pass's kernels (loaded at the first launch of a kernel of each translation unit
    // otherwise) by a side thread that starts with it — not inside the first pass of the job.  Joined by the entry points (join_prepare).
    static const bool no_prep = getenv("LDW_NO_PREPARE") != nullptr;
    if (!no_prep) {
        // (the streams here, synchronously: a side thread inside hipStreamCreate slowed the caller's upload of the alignment from 9.5 to 17 ms)
        if (int rc = ldw::ensure_streams(c)) return rc;
        c->prep_thread = std::thread([c] {
            int rc = LDW_OK;
            if (hipSetDevice(c->device) != hipSuccess) rc = LDW_ERR_HIP;
            if (rc == LDW_OK) {
                ldw::warm_mi();
                ldw::warm_apx();
                ldw::warm_pairs();
                ldw::warm_gemm_bits();
                ldw::warm_srp();
                ldw::warm_post();
            }
            if (rc != LDW_OK) c->prep_err = ldw_last_error();
            c->prep_rc = rc;
        });
    }
    *out = guard.release();
    return LDW_OK;
}

// r04: the pinned staging buffers of the all-pairs loop (hipHostMalloc: 0.2 ms per MB on this box; three of ~12 MB) and their device
// images, sized from the block geometry, by a second side thread — while the caller uploads the alignment and runs the Hamming GEMM.
// (tools/scratch/malloc_probe.cpp: hipMalloc itself is 0.02-0.25 ms whatever the size; what a first pass paid for was hipStreamCreate —
// now made with the context —, hipHostMalloc, the code-object loads and ensure_rows.)  Optional: everything is also made lazily.
int ldw_ctx_reserve(ldw_ctx *c, int64_t L, int64_t N, int64_t max_blk_sz) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(L > 0 && N > 0 && max_blk_sz > 0, LDW_ERR_ARG, "ldw_ctx_reserve: L, N and max_blk_sz must be positive");
    if (c->prep_thread2.joinable()) c->prep_thread2.join();   // an earlier reservation: finish it first
    static const bool no_prep = getenv("LDW_NO_PREPARE") != nullptr;
    if (no_prep) return LDW_OK;
    const int64_t blk = std::min<int64_t>(L, max_blk_sz);
    const int64_t nblk = (L + blk - 1) / blk;
    const int64_t nseg = std::max<int64_t>(1, std::min<int64_t>(c->knobs.span_on ? c->knobs.span_max : 1, nblk - 2));
    // the packed staging image of a span (prep_block): index, row and permutation lists of both sides, 48 bytes of intervals per to-side SNP
    const int64_t nt = blk * nseg, rows_f = blk * 5 / 4 + 512, rows_t = nt * 5 / 4 + 512;
    const size_t stage = (size_t)((blk + nt) * 12 + (rows_f + rows_t) * 9 + nt * 52 + (blk + 64) * 16 + 3 * (rows_t / 128 + 1) * (rows_f / 64 + 1) + 65536);   // (r06: + the band's tile list, at most 2 bytes per tile of the mask)
    const int64_t Npad = (N + ldw::KSTEP - 1) / ldw::KSTEP * ldw::KSTEP;
    c->prep_thread2 = std::thread([c, stage, Npad, blk, nseg] {
        int rc = LDW_OK;
        if (hipSetDevice(c->device) != hipSuccess) rc = LDW_ERR_HIP;
        if (rc == LDW_OK) rc = ldw::reserve_slot_buffers(c, Npad, blk, nseg);
        for (int k = 0; k < LDW_NSLOT && rc == LDW_OK; ++k) {
            if (c->pin[k].cap >= stage) continue;
            if ((rc = c->pin[k].reserve(stage * 2, "ldw_ctx_reserve")) != LDW_OK) break;
            if (c->dstage[k].reserve(stage * 2) != LDW_OK) rc = LDW_ERR_HIP;
        }
        if (rc != LDW_OK) c->prep_err2 = ldw_last_error();
        c->prep_rc2 = rc;
    });
    return LDW_OK;
}

int ldw_ctx_destroy(ldw_ctx *c) {
    if (!c) return LDW_OK;
    (void)hipSetDevice(c->device);
    (void)ldw::join_prepare(c);
    (void)ldw_tsv_join(c);
    (void)ldw_lr_stream_end(c, nullptr, nullptr, nullptr);
    for (hipStream_t s : {(hipStream_t)c->stream, (hipStream_t)c->gemm_stream, (hipStream_t)c->copy_stream, (hipStream_t)c->lr_st})
        if (s) (void)hipStreamSynchronize(s);
    {
        ldw::DrainedScope drained;   // every stream that could touch this context's blocks is idle: no device-wide synchronisation per released block
        ldw::fasta_release(c);
        ldw::out_release(c);
        ldw::grep_release(c);
        ldw::tsv_release(c);
        delete c;
    }
    ldw::ctx_count(-1);
    return LDW_OK;
}

int ldw_ctx_set_stream(ldw_ctx *c, void *s) {
    if (int rc = check_gpu(c)) return rc;
    // Everything the context has queued is done before its main stream changes: the old main stream, then the helper streams, which stay the
    // context's own whatever the main stream is (idle between calls; inside an open link pass they may hold work that waits for the old main
    // stream's events).  What the new stream runs is then ordered behind all of it by this host-side wait alone, so the stream may change
    // between any two calls, also between ldw_links_begin and ldw_links_end or while a tsv writer is open: the streaming writer waits for
    // events and copies on its own stream, the asynchronous one holds a host copy.  The side threads of ldw_ctx_create / ldw_ctx_reserve load
    // code objects and size buffers; they never touch a stream of the context and are not joined here.
    LDW_HIP(hipStreamSynchronize(c->stream));
    for (hipStream_t h : {(hipStream_t)c->gemm_stream, (hipStream_t)c->copy_stream, (hipStream_t)c->lr_st})
        if (h) LDW_HIP(hipStreamSynchronize(h));
    if (s) {
        c->stream.adopt((hipStream_t)s);
    } else {
        c->stream.destroy();
        LDW_HIP(c->stream.ensure(hipStreamNonBlocking));
    }
    return LDW_OK;
}

int ldw_ctx_sync(ldw_ctx *c) {
    if (int rc = check_gpu(c)) return rc;
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

int ldw_ctx_last_timing(ldw_ctx *c, double ms_out[4]) {
    LDW_REQUIRE(c && ms_out, LDW_ERR_ARG, "ldw_ctx_last_timing: null argument");
    for (int i = 0; i < 4; ++i) ms_out[i] = c->last_ms[i];
    return LDW_OK;
}

// ---- reports and switches: the entries that only read PassCounters or write Knobs (one needing a type of the MI unit stays in ldw_mi.hip) ----
// the first n of the eight pass counters (ldw_ctx_counters: 4, ldw_ctx_counters2: all)
static int ctx_counters(ldw_ctx *c, int64_t *out, int n, const char *who) {
    LDW_REQUIRE(c && out, LDW_ERR_ARG, "%s: null argument", who);
    const ldw::PassCounters &k = c->cnt;
    const int64_t all[8] = {k.spec_misses, 0 /* (the removed fused kernel's blocks) */, k.blocks_run, k.screen_violations, k.mixed_blocks, k.apx_blocks, k.apx_units_listed, k.apx_pairs_listed};
    std::copy(all, all + n, out);
    return LDW_OK;
}
int ldw_ctx_counters2(ldw_ctx *c, int64_t out[8]) { return ctx_counters(c, out, 8, "ldw_ctx_counters2"); }
int ldw_ctx_counters(ldw_ctx *c, int64_t out[4]) { return ctx_counters(c, out, 4, "ldw_ctx_counters"); }

int ldw_reset_speculation(ldw_ctx *c) {
    LDW_REQUIRE(c, LDW_ERR_ARG, "null context");
    c->spec.reset();
    return LDW_OK;
}

int ldw_path_report(ldw_ctx *c, int64_t out[8], char *gate, int capacity) {
    LDW_REQUIRE(c && out, LDW_ERR_ARG, "ldw_path_report: null argument");
    out[0] = c->cnt.apx_blocks;
    out[1] = c->cnt.mixed_blocks;
    out[2] = c->cnt.blocks_run - c->cnt.apx_blocks - c->cnt.mixed_blocks + c->cnt.spec_misses + c->cnt.generic_blocks;   // (blocks in generic POS order always take the plain path)
    out[3] = 0;   // (the removed fused kernel's blocks)
    out[4] = c->cnt.spec_misses;
    out[5] = c->cnt.probe_blocks;
    out[6] = c->cnt.apx_pairs_listed;
    out[7] = c->cnt.apx_units_listed;
    if (gate && capacity > 0) snprintf(gate, (size_t)capacity, "%s", c->apx.gate(c->wts.have_weights));
    return LDW_OK;
}

int ldw_pair_form_report(ldw_ctx *c, int64_t out[5]) {
    LDW_REQUIRE(c && out, LDW_ERR_ARG, "ldw_pair_form_report: null argument");
    for (int i = 0; i < 5; ++i) out[i] = c->cnt.form_launches[i];
    return LDW_OK;
}

int ldw_pair_kernel_report(ldw_ctx *c, int64_t out[2]) {
    LDW_REQUIRE(c && out, LDW_ERR_ARG, "ldw_pair_kernel_report: null argument");
    for (int i = 0; i < 2; ++i) out[i] = c->cnt.pair_kernel_launches[i];
    return LDW_OK;
}

int ldw_set_prune(ldw_ctx *c, int on) {
    LDW_REQUIRE(c, LDW_ERR_ARG, "null context");
    c->knobs.prune = on != 0;
    return LDW_OK;
}

int ldw_prune_report(ldw_ctx *c, int64_t out[4]) {
    LDW_REQUIRE(c && out, LDW_ERR_ARG, "ldw_prune_report: null argument");
    out[0] = c->cnt.sorted_blocks;
    out[1] = c->cnt.apx_waves_skipped;
    out[2] = c->cnt.apx_waves_total;
    out[3] = c->knobs.prune ? 1 : 0;
    return LDW_OK;
}

int ldw_snp_bounds(ldw_ctx *c, double *out, int64_t capacity) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(out, LDW_ERR_ARG, "ldw_snp_bounds: null argument");
    if (int rc = ldw::ensure_rows(c)) return rc;
    LDW_REQUIRE(capacity >= 4 * c->L, LDW_ERR_ARG, "ldw_snp_bounds: capacity %lld < 4 L = %lld", (long long)capacity, (long long)(4 * c->L));
    LDW_HIP(hipMemcpyAsync(out, c->rows.snp_sup.p, (size_t)c->L * 32, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

int ldw_set_select(ldw_ctx *c, int mode) {
    LDW_REQUIRE(c && (mode == 0 || mode == 1), LDW_ERR_ARG, "ldw_set_select: mode must be 0 (auto) or 1 (radix sorts)");
    c->knobs.select_mode = mode;
    return LDW_OK;
}

int ldw_set_path(ldw_ctx *c, int mode) {
    LDW_REQUIRE(c && mode >= 0 && mode <= 2, LDW_ERR_ARG, "ldw_set_path: mode must be 0 (auto), 1 (limb GEMM paths) or 2 (approximate GEMM path)");
    c->knobs.path_mode = mode;
    return LDW_OK;
}

int ldw_apx_info(ldw_ctx *c, double out[6]) {
    LDW_REQUIRE(c && out, LDW_ERR_ARG, "ldw_apx_info: null argument");
    out[0] = c->apx.apx_ok ? 1.0 : 0.0;
    out[1] = c->apx.apx_delta;
    out[2] = (double)c->apx.n_classes;
    out[3] = (double)c->apx.n_pop_segs;
    out[4] = (double)c->apx.apx_transitions;
    out[5] = (double)c->apx.apx_e_last;
    return LDW_OK;
}

int ldw_gemm_stats(ldw_ctx *c, double out[6], int reset) {
    LDW_REQUIRE(c && out, LDW_ERR_ARG, "ldw_gemm_stats: null argument");
    for (int k = 0; k < 6; ++k) {
        out[k] = c->cnt.gemm_stat[k];
        if (reset) c->cnt.gemm_stat[k] = 0;
    }
    return LDW_OK;
}

int ldw_set_engine(ldw_ctx *c, int engine) {
    LDW_REQUIRE(c, LDW_ERR_ARG, "null context");
    LDW_REQUIRE(engine == LDW_ENGINE_MFMA || engine == LDW_ENGINE_HIST || engine == LDW_ENGINE_HIST_STATES, LDW_ERR_ARG, "unknown engine %d", engine);
    LDW_REQUIRE(engine != LDW_ENGINE_HIST_STATES, LDW_ERR_STATE,
                "LDW_ENGINE_HIST_STATES: the byte-state histogram kernel (formerly the LDW_EXPERIMENTS build's) was measured ~200x slower and has been removed");
    c->knobs.engine = engine;
    return LDW_OK;
}

int ldw_overflow_report(ldw_ctx *c, int64_t out[4]) {
    LDW_REQUIRE(c && out, LDW_ERR_ARG, "ldw_overflow_report: null argument");
    out[0] = c->cnt.pair_list_overflows;
    out[1] = c->cnt.maybe_overflows;
    out[2] = c->spec.maybe_off ? 1 : 0;
    out[3] = c->cnt.maybe_entries;
    return LDW_OK;
}

int ldw_span_report(ldw_ctx *c, int64_t out[4]) {
    LDW_REQUIRE(c && out, LDW_ERR_ARG, "ldw_span_report: null argument");
    out[0] = c->cnt.span_items;
    out[1] = c->cnt.span_blocks;
    out[2] = c->cnt.span_fallbacks;
    out[3] = c->knobs.span_on ? 1 : 0;
    return LDW_OK;
}

int ldw_set_span(ldw_ctx *c, int on, int max_blocks) {
    LDW_REQUIRE(c && (max_blocks == 0 || (max_blocks >= 2 && max_blocks <= LDW_SPAN_MAX)), LDW_ERR_ARG, "ldw_set_span: max_blocks must be 0 or 2..%d", LDW_SPAN_MAX);
    LDW_REQUIRE(!(on & 6), LDW_ERR_STATE, "ldw_set_span: corner spans / split diagonal blocks (bits 1, 2; formerly the LDW_EXPERIMENTS build's) were measured slower and have been removed");
    c->knobs.span_on = on != 0;
    if (max_blocks) c->knobs.span_max = max_blocks;
    return LDW_OK;
}

int ldw_set_overlap(ldw_ctx *c, int on) {
    LDW_REQUIRE(c, LDW_ERR_ARG, "null context");
    c->knobs.overlap = on != 0;
    return LDW_OK;
}

int ldw_set_screen(ldw_ctx *c, int mode) {
    LDW_REQUIRE(c && mode >= 0 && mode <= 2, LDW_ERR_ARG, "ldw_set_screen: mode must be 0, 1 or 2");
    c->knobs.screen = mode;
    return LDW_OK;
}

int ldw_set_mixed(ldw_ctx *c, int on) {
    LDW_REQUIRE(c, LDW_ERR_ARG, "null context");
    c->knobs.mixed = on != 0;
    return LDW_OK;
}

int ldw_set_fused(ldw_ctx *c, int on) {
    LDW_REQUIRE(!on, LDW_ERR_STATE, "ldw_set_fused(1): the fused GEMM + epilogue kernel (formerly the LDW_EXPERIMENTS build's) was measured slower and has been removed");
    LDW_REQUIRE(c, LDW_ERR_ARG, "null context");
    return LDW_OK;
}

// ---- (1) ACGTN2num --------------------------------------------------------------------------------
int ldw_acgtn2num_dev(ldw_ctx *c, double *nv_dev, const char *ref_dev, int64_t L) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(nv_dev && ref_dev && L >= 0, LDW_ERR_ARG, "ldw_acgtn2num_dev: bad argument");
    if (L == 0) return LDW_OK;
    hipLaunchKernelGGL(k_acgtn2num, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, c->stream, nv_dev, ref_dev, L);
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

int ldw_acgtn2num(ldw_ctx *c, double *nv, const char *ref, int64_t L, int /*ncores*/) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(nv && ref && L >= 0, LDW_ERR_ARG, "ldw_acgtn2num: bad argument");
    if (L == 0) return LDW_OK;
    if (int rc = c->scratch.reserve((size_t)L * 41 + 64)) return rc;
    double *d_nv = c->scratch.as<double>();
    char *d_ref = reinterpret_cast<char *>(d_nv + 5 * L);
    LDW_HIP(hipMemcpyAsync(d_nv, nv, (size_t)L * 40, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(d_ref, ref, (size_t)L, hipMemcpyHostToDevice, c->stream));
    if (int rc = ldw_acgtn2num_dev(c, d_nv, d_ref, L)) return rc;
    LDW_HIP(hipMemcpyAsync(nv, d_nv, (size_t)L * 40, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

// ---- (3) fastHadamard ---------------------------------------------------------------------------
int ldw_fast_hadamard(ldw_ctx *c, double *MI, const double *den, const double *uq, const double *pxy,
                      const double *pxpy, const double *RXY, const double *pXrX, const double *pYrY, int64_t n,
                      int on_device) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(MI && den && uq && pxy && pxpy && RXY && pXrX && pYrY && n >= 0, LDW_ERR_ARG,
                "ldw_fast_hadamard: bad argument");
    if (n == 0) return LDW_OK;
    const double *src[8] = {MI, den, uq, pxy, pxpy, RXY, pXrX, pYrY};
    const double *dv[8];
    if (on_device) {
        for (int i = 0; i < 8; ++i) dv[i] = src[i];
    } else {
        if (int rc = c->scratch.reserve((size_t)n * 64)) return rc;
        for (int i = 0; i < 8; ++i) {
            double *d = c->scratch.as<double>() + (size_t)i * n;
            LDW_HIP(hipMemcpyAsync(d, src[i], (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
            dv[i] = d;
        }
    }
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(k_fast_hadamard, dim3((unsigned)(blocks > 65535 * 16 ? 65535 * 16 : blocks)), dim3(256), 0,
                       c->stream, const_cast<double *>(dv[0]), dv[1], dv[2], dv[3], dv[4], dv[5], dv[6], dv[7], n);
    LDW_HIP(hipGetLastError());
    if (!on_device) {
        LDW_HIP(hipMemcpyAsync(MI, dv[0], (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
    }
    return LDW_OK;
}

// ---- alignment residency ------------------------------------------------------------------------
extern "C++" {   // (ldw_fasta.cpp sets the shape too)
int ldw::set_dims(ldw_ctx *c, int64_t L, int64_t N) {
    LDW_REQUIRE(L > 0 && N > 0, LDW_ERR_ARG, "alignment must be non-empty (L=%lld N=%lld)", (long long)L, (long long)N);
    LDW_REQUIRE(L < (int64_t)1 << 27, LDW_ERR_ARG, "L too large (%lld)", (long long)L);
    c->L = L;
    c->N = N;
    c->Npad = (N + KSTEP - 1) / KSTEP * KSTEP;
    c->KW = c->Npad / 64;
    c->new_shape();
    return c->states.reserve((size_t)L * c->Npad);
}
}

int ldw_set_alignment(ldw_ctx *c, const uint8_t *states, int64_t L, int64_t N, int on_device) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(states, LDW_ERR_ARG, "ldw_set_alignment: states is null");
    if (int rc = set_dims(c, L, N)) return rc;
    const uint8_t *src = states;
    if (!on_device) {
        if (int rc = c->scratch.reserve((size_t)L * N)) return rc;
        LDW_HIP(hipMemcpyAsync(c->scratch.p, states, (size_t)L * N, hipMemcpyHostToDevice, c->stream));
        src = c->scratch.as<uint8_t>();
    }
    hipLaunchKernelGGL(k_pad_states, dim3((unsigned)L), dim3(256), 0, c->stream, src, c->states.as<uint8_t>(), L, N, c->Npad);
    LDW_HIP(hipGetLastError());
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

int ldw_get_alignment(ldw_ctx *c, uint8_t *out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(out && ldw::have_alignment(c), LDW_ERR_STATE, "ldw_get_alignment: no alignment resident");
    if (int rc = c->scratch.reserve((size_t)c->L * c->N)) return rc;
    hipLaunchKernelGGL(k_unpad_states, dim3((unsigned)c->L), dim3(256), 0, c->stream, c->states.as<uint8_t>(), c->scratch.as<uint8_t>(),
                       c->L, c->N, c->Npad);
    LDW_HIP(hipGetLastError());
    LDW_HIP(hipMemcpyAsync(out, c->scratch.p, (size_t)c->L * c->N, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

int ldw_state_counts(ldw_ctx *c, int32_t *counts_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(counts_out && ldw::have_alignment(c), LDW_ERR_STATE, "ldw_state_counts: no alignment resident");
    if (int rc = ldw::launch_state_counts(c)) return rc;
    // stored [L][5] row-major == 5 x L column-major (ACGTN_table layout)
    LDW_HIP(hipMemcpyAsync(counts_out, c->rows.counts.p, (size_t)c->L * 20, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

int ldw_alignment_scan(ldw_ctx *c, const char *chars, int64_t N, int64_t L_total, int32_t *allele_counts_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(chars && allele_counts_out && N > 0 && L_total > 0, LDW_ERR_ARG, "ldw_alignment_scan: bad argument");
    const size_t cb = (size_t)N * L_total;
    if (int rc = c->chars.reserve(cb)) return rc;
    if (int rc = c->scratch.reserve((size_t)L_total * 20)) return rc;
    LDW_HIP(hipMemcpyAsync(c->chars.p, chars, cb, hipMemcpyHostToDevice, c->stream));
    c->cN = N;
    c->cL = L_total;
    hipLaunchKernelGGL(k_column_counts, dim3((unsigned)((L_total + 255) / 256)), dim3(256), 0, c->stream, c->chars.as<char>(),
                       N, L_total, c->scratch.as<int32_t>());
    LDW_HIP(hipGetLastError());
    LDW_HIP(hipMemcpyAsync(allele_counts_out, c->scratch.p, (size_t)L_total * 20, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

int ldw_encode_alignment(ldw_ctx *c, const char *chars, int64_t N, int64_t L_total, const int32_t *pos, int64_t n_pos,
                         int32_t *acgtn_table_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(pos && N > 0 && L_total > 0 && n_pos > 0, LDW_ERR_ARG, "ldw_encode_alignment: bad argument");
    LDW_REQUIRE(chars || (c->chars.p && c->cN == N && c->cL == L_total), LDW_ERR_STATE,
                "ldw_encode_alignment: chars is NULL and no alignment of that shape was scanned");
    for (int64_t i = 0; i < n_pos; ++i)
        LDW_REQUIRE(pos[i] >= 1 && pos[i] <= L_total, LDW_ERR_ARG, "ldw_encode_alignment: pos[%lld]=%d outside 1..%lld",
                    (long long)i, pos[i], (long long)L_total);
    if (int rc = set_dims(c, n_pos, N)) return rc;
    const size_t cb = (size_t)N * L_total;
    const char *d_chars;
    if (chars) {
        if (int rc = c->chars.reserve(cb)) return rc;
        LDW_HIP(hipMemcpyAsync(c->chars.p, chars, cb, hipMemcpyHostToDevice, c->stream));
        c->cN = N;
        c->cL = L_total;
    }
    d_chars = c->chars.as<char>();
    if (int rc = c->scratch.reserve((size_t)n_pos * 4)) return rc;
    int32_t *d_pos = c->scratch.as<int32_t>();
    LDW_HIP(hipMemcpyAsync(d_pos, pos, (size_t)n_pos * 4, hipMemcpyHostToDevice, c->stream));
    dim3 grid((unsigned)((n_pos + 63) / 64), (unsigned)((c->Npad + 63) / 64));
    hipLaunchKernelGGL(k_encode, grid, dim3(256), 0, c->stream, d_chars, N, L_total, d_pos, n_pos,
                       c->states.as<uint8_t>(), c->Npad);
    LDW_HIP(hipGetLastError());
    LDW_HIP(hipStreamSynchronize(c->stream));
    if (acgtn_table_out) return ldw_state_counts(c, acgtn_table_out);
    return LDW_OK;
}

// ---- weights / meta -------------------------------------------------------------------------------
int ldw_set_weights(ldw_ctx *c, const double *hdw, int64_t N, int nlimbs) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(ldw::have_alignment(c), LDW_ERR_STATE, "ldw_set_weights: set the alignment first");
    LDW_REQUIRE(hdw && N == c->N, LDW_ERR_ARG, "ldw_set_weights: hdw has %lld entries, alignment has %lld sequences",
                (long long)N, (long long)c->N);
    if (nlimbs == 0) nlimbs = 5;
    LDW_REQUIRE(nlimbs >= 1 && nlimbs <= 6, LDW_ERR_ARG, "ldw_set_weights: nlimbs must be 1..6");
    if (const char *dz = getenv("LDW_DEBUG_ZERO")) {   // debugging aid: zero whole buffer groups when the weights change (which stale tail does a later, smaller problem read?)
        const int mask = atoi(dz);
        if (int rc = join_prepare(c)) return rc;
        LDW_HIP(hipDeviceSynchronize());
        std::vector<ldw::DevBuf *> g;
        if (mask & 1) g.insert(g.end(), {&c->apx.dig_a, &c->apx.dig_b, &c->apx.apx_shift, &c->wts.seq_perm, &c->wts.digits, &c->wts.vfixed});
        if (mask & 2) g.insert(g.end(), {&c->apx.pop_segs, &c->apx.pop_wbeg, &c->apx.pop_vpos, &c->rows.slot_papx});
        if (mask & 4)
            for (int k = 0; k < LDW_NSLOT; ++k) g.insert(g.end(), {&c->panel[k][0], &c->panel[k][1], &c->Gapx[k]});
        if (mask & 8)
            for (int k = 0; k < LDW_NSLOT; ++k)
                g.insert(g.end(), {&c->apx_bins[k], &c->apx_clean[k], &c->apx_mini[k], &c->apx_units[k], &c->apx_packs[k], &c->pairs[k]});
        for (int k = 0; k < LDW_NSLOT; ++k) {
            ldw::DevBuf *one[6] = {&c->apx_bins[k], &c->apx_clean[k], &c->apx_mini[k], &c->apx_units[k], &c->apx_packs[k], &c->pairs[k]};
            for (int q = 0; q < 6; ++q)
                if (mask & (64 << q)) g.push_back(one[q]);
        }
        if (mask & 16)
            g.insert(g.end(), {&c->rows.Mbits, &c->rows.row0, &c->rows.slot_meta, &c->rows.slot_pfix, &c->rows.slot_pfix_hi, &c->rows.counts, &c->rows.pfix_state, &c->rows.snp_sup, &c->packs, &c->glo, &c->lo_rows});
        if (mask & 32) {
            g.insert(g.end(), {&c->G, &c->G2, &c->G3, &c->MIblk, &c->rowlist_f, &c->rowlist_t, &c->idx_f, &c->idx_t, &c->lrow_f, &c->lrow_t, &c->perm_f, &c->perm_t, &c->scr_units, &c->epi_rest, &c->colcnt,
                               &c->cand_key2, &c->cand_val2, &c->sel_bitmap, &c->sel_chunks, &c->sel_prefix, &c->scratch, &c->small, &c->pair_sums, &c->spec.tab11[0], &c->spec.tab11[1], &c->miss_key,
                               &c->miss_val});
            for (int k = 0; k < LDW_NSLOT; ++k) g.insert(g.end(), {&c->hist[k], &c->cand_key[k], &c->cand_val[k], &c->dstage[k]});
        }
        for (ldw::DevBuf *b : g)
            if (b->p) LDW_HIP(hipMemsetAsync(b->p, 0, b->cap, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
    }
    std::vector<double> v((size_t)N);
    long double neff = 0.0L, vsum = 0.0L;
    double vmax = 0;
    for (int64_t s = 0; s < N; ++s) {
        LDW_REQUIRE(std::isfinite(hdw[s]) && hdw[s] >= 0, LDW_ERR_ARG, "ldw_set_weights: hdw[%lld] = %g is not a finite non-negative weight",
                    (long long)s, hdw[s]);
        const double sq = std::sqrt(hdw[s]);
        v[s] = sq * sq;  // the reference multiplies two sqrt(w)-scaled one-hots (R/computePairwiseMI.R:238,391)
        neff += (long double)hdw[s];
        vsum += (long double)v[s];
        if (v[s] > vmax) vmax = v[s];
    }
    LDW_REQUIRE(vmax > 0, LDW_ERR_ARG, "ldw_set_weights: all weights are zero");
    // fixed point: V_s = round(v_s * 2^F) must fit nlimbs balanced base-256 digits and every sum of V_s must
    // stay below 2^52 so that counts convert to double exactly.
    const double lim_digits = 0.99 * std::ldexp(1.0, 8 * nlimbs - 1) / vmax;
    const double lim_sum = std::ldexp(1.0, 52) / (double)vsum;
    int F = (int)std::floor(std::log2(std::fmin(lim_digits, lim_sum)));
    bool unit = true;  // all weights exactly 1 (unweighted counts): F = 0 is exact with one limb
    for (int64_t s = 0; s < N; ++s) unit = unit && (v[s] == 1.0);
    if (unit) F = 0;
    c->wts.nlimbs = nlimbs;
    c->wts.frac_bits = F;
    c->wts.neff = (double)neff;
    c->wts.h_hdw.assign(hdw, hdw + N);
    c->wts.h_vfixed.assign((size_t)c->Npad, 0);
    std::vector<int8_t> dseq((size_t)nlimbs * c->Npad, 0);   // digits by sequence
    int64_t total = 0;
    for (int64_t s = 0; s < N; ++s) {
        int64_t V = (int64_t)std::llround(std::ldexp(v[s], F));
        c->wts.h_vfixed[s] = V;
        total += V;
        int64_t rem = V;
        for (int j = 0; j < nlimbs; ++j) {
            int64_t d = ((rem + 128) & 255) - 128;  // balanced digit in [-128, 127]
            dseq[(size_t)j * c->Npad + s] = (int8_t)d;
            rem = (rem - d) / 256;
        }
        LDW_REQUIRE(rem == 0, LDW_ERR_ARG, "ldw_set_weights: internal: weight %g does not fit %d limbs at F=%d", v[s], nlimbs, F);
    }
    c->wts.total_fixed = total;
    // Mixed-precision path (5 limbs only): the block-wide GEMM carries the 3 high limbs, V = V_hi * 2^16 + V_lo.
    // lo_abs_sum = sum |V_lo| 2^-F bounds what the low limbs can add to any joint sum.
    c->wts.h_vfixed_hi.assign((size_t)c->Npad, 0);
    c->wts.total_fixed_hi = 0;
    c->wts.lo_abs_sum = 0;
    if (nlimbs == 5) {
        long double lo_abs = 0;
        for (int64_t s = 0; s < N; ++s) {
            const int64_t lo = (int64_t)dseq[s] + 256 * (int64_t)dseq[(size_t)c->Npad + s];
            c->wts.h_vfixed_hi[s] = (c->wts.h_vfixed[s] - lo) / 65536;   // exact: the remainder is what limbs 2..4 encode
            c->wts.total_fixed_hi += c->wts.h_vfixed_hi[s];
            lo_abs += (long double)(lo < 0 ? -lo : lo);
        }
        c->wts.lo_abs_sum = (double)(lo_abs * (long double)std::ldexp(1.0, -F));
    }
    // Position order of the bit rows: ascending weight (ties by sequence), padding last.  A sum over sequences does not
    // care about their order; this one makes the sequences of one weight CLASS contiguous (class-wise popcounts of the
    // approximate-GEMM path) and lets consecutive 128-position macro steps share a block exponent.
    {
        std::vector<int32_t> order((size_t)N);
        for (int64_t s = 0; s < N; ++s) order[(size_t)s] = (int32_t)s;
        std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return c->wts.h_vfixed[x] < c->wts.h_vfixed[y]; });
        c->wts.h_seq_perm.assign((size_t)c->Npad, -1);
        for (int64_t q = 0; q < N; ++q) c->wts.h_seq_perm[(size_t)q] = order[(size_t)q];
    }
    std::vector<int8_t> dig((size_t)nlimbs * c->Npad, 0);   // digits by position
    for (int j = 0; j < nlimbs; ++j)
        for (int64_t q = 0; q < N; ++q) dig[(size_t)j * c->Npad + q] = dseq[(size_t)j * c->Npad + c->wts.h_seq_perm[(size_t)q]];
    if (int rc = c->wts.seq_perm.reserve((size_t)c->Npad * 4)) return rc;
    LDW_HIP(hipMemcpyAsync(c->wts.seq_perm.p, c->wts.h_seq_perm.data(), (size_t)c->Npad * 4, hipMemcpyHostToDevice, c->stream));
    if (int rc = prepare_apx_weights(c)) return rc;
    if (int rc = c->wts.digits.reserve(dig.size())) return rc;
    if (int rc = c->wts.vfixed.reserve((size_t)c->Npad * 8)) return rc;
    LDW_HIP(hipMemcpyAsync(c->wts.digits.p, dig.data(), dig.size(), hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(c->wts.vfixed.p, c->wts.h_vfixed.data(), (size_t)c->Npad * 8, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    c->new_weights();
    return LDW_OK;
}

int ldw_set_snp_meta(ldw_ctx *c, const double *r, const uint8_t *uqe, const int32_t *POS, const int32_t *paint, double g) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(ldw::have_alignment(c), LDW_ERR_STATE, "ldw_set_snp_meta: set the alignment first");
    if (int rc = ldw_tsv_join(c)) return rc;   // (a pending asynchronous table reads the positions this call replaces)
    LDW_REQUIRE(r && uqe && POS, LDW_ERR_ARG, "ldw_set_snp_meta: null argument");
    LDW_REQUIRE(g > 0, LDW_ERR_ARG, "ldw_set_snp_meta: genome length g must be positive (snp.dat$g)");
    const int64_t L = c->L;
    for (int64_t i = 0; i < L * 5; ++i) LDW_REQUIRE(uqe[i] <= 1, LDW_ERR_ARG, "ldw_set_snp_meta: uqe must be 0/1");
    if (int rc = c->meta.r.reserve((size_t)L * 8)) return rc;
    if (int rc = c->meta.uqe.reserve((size_t)L * 5)) return rc;
    if (int rc = c->meta.POS.reserve((size_t)L * 4)) return rc;
    if (int rc = c->meta.paint.reserve((size_t)L * 4)) return rc;
    LDW_HIP(hipMemcpyAsync(c->meta.r.p, r, (size_t)L * 8, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(c->meta.uqe.p, uqe, (size_t)L * 5, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(c->meta.POS.p, POS, (size_t)L * 4, hipMemcpyHostToDevice, c->stream));
    if (paint) LDW_HIP(hipMemcpyAsync(c->meta.paint.p, paint, (size_t)L * 4, hipMemcpyHostToDevice, c->stream));
    else LDW_HIP(hipMemsetAsync(c->meta.paint.p, 0, (size_t)L * 4, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    c->meta.h_r.assign(r, r + L);
    c->meta.r_min = r[0];
    for (int64_t i = 1; i < L; ++i) c->meta.r_min = r[i] < c->meta.r_min ? r[i] : c->meta.r_min;
    c->meta.set_positions(POS, L);
    if (paint) c->meta.h_paint.assign(paint, paint + L);
    else c->meta.h_paint.assign((size_t)L, 0);
    c->meta.paint_min = c->meta.paint_max = 0;
    if (paint) {
        c->meta.paint_min = c->meta.paint_max = paint[0];
        for (int64_t i = 1; i < L; ++i) {
            c->meta.paint_min = paint[i] < c->meta.paint_min ? paint[i] : c->meta.paint_min;
            c->meta.paint_max = paint[i] > c->meta.paint_max ? paint[i] : c->meta.paint_max;
        }
    }
    c->meta.g = g;
    c->new_meta();
    // r04: with the alignment and the weights in place the row map (indicator rows, marginals, per-SNP bounds: ensure_rows, ~9 ms at C4) is
    // built HERE — it belongs to handing over the data — instead of lazily inside the first block loop; a later ldw_set_weights
    // invalidates it again and the next pass rebuilds it
    if (c->L > 0 && c->wts.have_weights) return ldw::ensure_rows(c);
    return LDW_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------
// row map: which (SNP, state) pairs get an indicator row
// ------------------------------------------------------------------------------------------------
namespace ldw {

// ------------------------------------------------------------------------------------------------
// k_snp_sup: how large can the MI of SNP a get, whatever its partner looks like?  With the marginals p_x of a fixed, the MI of
// R/computePairwiseMI.R:390-398 is
//     F(n) = 1/den sum_xy q_xy ln(q_xy den / D_xy),   q = n + 1/2,   D_xy = p_x pY_y + RXY + p_x r_a/2 + pY_y r_b/2,   pY_y = sum_x n_xy
// over the joint tables n >= 0 with row sums p_x.  q and D are affine in n and q ln(q / D) is jointly convex (relative entropy),
// so F is convex on that polytope — a product of simplices — and takes its maximum at a vertex: every state of a sends ALL
// its weight to one state of the partner.  For a partner with k flagged states that is k^(states of a) tables: enumerate them.
// F falls as RXY grows; the reference's scrambled RXY (quirk Q1) is r r' / 4 of two other SNPs of the block, at least
// r_min^2 / 4: the m = 1 values use that floor.  Near-singleton sites (most of a real alignment) come out below any threshold
// a long-range link has to reach: the screen and the approximate GEMM drop their pairs without looking at them
// (apx_tile_prunable, k_mi_screen).  One thread per SNP, once per weighting.
// ------------------------------------------------------------------------------------------------
__device__ double mi_vertex_sup(const double *p, int ka, int kb, double neff, double rxy) {
    const double den = neff + 0.5 * ka * kb, rX = 0.5 * ka, rY = 0.5 * kb;
    int nv = 1;
    for (int x = 0; x < ka; ++x) nv *= kb;
    double best = -1e300;
    for (int v = 0; v < nv; ++v) {
        int phi[3];
        double pY[3] = {0.0, 0.0, 0.0};
        int t = v;
        for (int x = 0; x < ka; ++x) {
            phi[x] = t % kb;
            t /= kb;
            pY[phi[x]] += p[x];
        }
        double F = 0.0;
        for (int x = 0; x < ka; ++x)
            for (int y = 0; y < kb; ++y) {
                const double q = (phi[x] == y ? p[x] : 0.0) + 0.5;
                const double D = p[x] * pY[y] + rxy + p[x] * rX + pY[y] * rY;
                if (!(D > 0.0)) return 1e300;   // (degenerate r: no statement)
                F += q * log(q * den / D);
            }
        F /= den;
        if (!(F == F)) return 1e300;
        best = F > best ? F : best;
    }
    return best;
}

__global__ __launch_bounds__(256) void k_snp_sup(int64_t L, const uint32_t *__restrict__ slot_meta, const int64_t *__restrict__ slot_pfix,
                                                 const double *__restrict__ r, double scale, double neff, double r_min, double *__restrict__ sup) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= L) return;
    const uint32_t m = slot_meta[a];
    const int n = (int)(m & 7), ka = n + 1;
    double out[4] = {1e300, 1e300, 1e300, 1e300};
    const uint32_t full = (2u << n) - 1u;
    if ((ka == 2 || ka == 3) && ((m >> 3) & full) == full && r[a] == (double)ka) {
        double p[3] = {0.0, 0.0, 0.0};
        double minor = 0.0;
        for (int x = 0; x < ka; ++x) {
            p[x] = (double)slot_pfix[a * 5 + x] * scale;
            if (x < n) minor += p[x];
        }
        // a SNP with any sizeable minor state reaches every threshold of interest: not worth the enumeration (+inf is the safe answer)
        if (minor < 0.05 * neff + 4.0)
            for (int kb = 2; kb <= 3; ++kb) {
                out[kb - 2] = mi_vertex_sup(p, ka, kb, neff, 0.25 * ka * kb) * (1.0 + 1e-12) + 1e-12;
                const double rfloor = 0.25 * r_min * r_min;
                out[2 + kb - 2] = mi_vertex_sup(p, ka, kb, neff, rfloor < 0.25 * ka * kb ? rfloor : 0.25 * ka * kb) * (1.0 + 1e-12) + 1e-12;
            }
    }
    for (int k = 0; k < 4; ++k) sup[a * 4 + k] = out[k];
}

// dst (int64 [L][5]) = the fixed-point marginals of the per-sequence weights w [Npad] by slot (h_slot_meta), shifted right by `shift`; synchronous
static int slot_marginals(ldw_ctx *c, const std::vector<int64_t> &w, int shift, ldw::DevBuf &dst, const char *what) {
    const int64_t L = c->L, Npad = c->Npad;
    ldw::DevBuf d_w, d_p, d_cnt;
    if (int rc = d_w.reserve((size_t)Npad * 8)) return rc;
    if (int rc = d_p.reserve((size_t)L * 40)) return rc;
    if (int rc = d_cnt.reserve((size_t)L * 20)) return rc;
    if (int rc = dst.reserve((size_t)L * 40)) return rc;
    hipError_t he = hipMemcpyAsync(d_w.p, w.data(), (size_t)Npad * 8, hipMemcpyHostToDevice, c->stream);
    hipLaunchKernelGGL(k_counts_marginals, dim3((unsigned)((L + 3) / 4)), dim3(256), 0, c->stream, c->states.as<uint8_t>(), L, Npad, d_w.as<int64_t>(),
                       d_cnt.as<int32_t>(), d_p.as<int64_t>());
    std::vector<int64_t> by_state((size_t)L * 5), by_slot((size_t)L * 5, 0);
    if (he == hipSuccess) he = hipMemcpyAsync(by_state.data(), d_p.p, (size_t)L * 40, hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    if (he != hipSuccess) return ldw::hip_fail(he, what, __FILE__, __LINE__);
    for (int64_t a = 0; a < L; ++a) {
        const uint32_t m = c->rows.h_slot_meta[a];
        const int n = (int)(m & 7);
        for (int i = 0; i <= n; ++i) by_slot[a * 5 + i] = by_state[a * 5 + ((m >> (8 + 3 * i)) & 7)] >> shift;
    }
    LDW_HIP(hipMemcpyAsync(dst.p, by_slot.data(), (size_t)L * 40, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

// Marginals of the high-limb weights, by slot, for the screen of the MIXED-precision path — made when a block first takes that path (r04: the
// default path never does, and building them eagerly cost 2.5 ms of every job's ldw_set_snp_meta).
int ensure_hi_marginals(ldw_ctx *c) {
    if (c->rows.hi_ready || c->wts.nlimbs != 5) return LDW_OK;
    LDW_REQUIRE((int64_t)c->rows.h_slot_meta.size() == c->L, LDW_ERR_STATE, "ensure_hi_marginals: the row map has not been built");
    if (int rc = slot_marginals(c, c->wts.h_vfixed_hi, 0, c->rows.slot_pfix_hi, "high-limb marginals")) return rc;
    c->rows.hi_ready = true;
    return LDW_OK;
}

int ensure_rows(ldw_ctx *c) {
    if (c->rows.rows_ready) return LDW_OK;
    const auto t_rows0 = HostClock::now();
    auto lap = [&](const char *what) {
        if (!host_timing()) return;
        (void)hipStreamSynchronize(c->stream);
        fprintf(stderr, "[ldw] ensure_rows: %.2f ms at %s\n", HostClock::ms(t_rows0, HostClock::now()), what);
    };
    LDW_REQUIRE(ldw::have_alignment(c) && c->wts.have_weights && c->meta.have_meta, LDW_ERR_STATE,
                "MI needs the alignment, the weights and the SNP meta data to be set first");
    const int64_t L = c->L, Npad = c->Npad;
    if (int rc = c->rows.counts.reserve((size_t)L * 20)) return rc;
    if (int rc = c->rows.slot_pfix.reserve((size_t)L * 40)) return rc;
    if (int rc = c->rows.pfix_state.reserve((size_t)L * 40)) return rc;
    int64_t *d_pfix_state = c->rows.pfix_state.as<int64_t>();  // [L][5] by state
    hipLaunchKernelGGL(k_counts_marginals, dim3((unsigned)((L + 3) / 4)), dim3(256), 0, c->stream,
                       c->states.as<uint8_t>(), L, Npad, c->wts.vfixed.as<int64_t>(), c->rows.counts.as<int32_t>(), d_pfix_state);
    LDW_HIP(hipGetLastError());
    c->rows.h_counts.resize((size_t)L * 5);
    std::vector<int64_t> pfs((size_t)L * 5);
    std::vector<uint8_t> uqe((size_t)L * 5);
    LDW_HIP(hipMemcpyAsync(c->rows.h_counts.data(), c->rows.counts.p, (size_t)L * 20, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(pfs.data(), d_pfix_state, (size_t)L * 40, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(uqe.data(), c->meta.uqe.p, (size_t)L * 5, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    lap("counts + exact marginals fetched");

    // Slots of SNP a: one per state that is present (count > 0) or flagged in uqe.  The most frequent
    // present state is the "drop" slot: it gets no indicator row, its joint cells follow from the
    // marginals by exact integer subtraction.  Rows are the remaining slots in increasing state order.
    c->rows.h_row0.assign((size_t)L + 1, 0);
    std::vector<uint32_t> meta((size_t)L);
    std::vector<int64_t> spf((size_t)L * 5, 0);
    std::vector<int32_t> rowinfo;
    rowinfo.reserve((size_t)L * 2);
    for (int64_t a = 0; a < L; ++a) {
        const int32_t *cnt = &c->rows.h_counts[a * 5];
        int drop = -1;
        for (int x = 0; x < 5; ++x)
            if (cnt[x] > 0 && (drop < 0 || cnt[x] > cnt[drop])) drop = x;
        LDW_REQUIRE(drop >= 0, LDW_ERR_ARG, "SNP %lld has no valid state (all sequences outside 0..4)", (long long)a);
        uint32_t m = 0;
        int nrows = 0;
        for (int x = 0; x < 5; ++x) {
            if (x == drop) continue;
            if (cnt[x] > 0 || uqe[a * 5 + x]) {
                m |= (uint32_t)uqe[a * 5 + x] << (3 + nrows);
                m |= (uint32_t)x << (8 + 3 * nrows);
                spf[a * 5 + nrows] = pfs[a * 5 + x];
                rowinfo.push_back((int32_t)(a * 8 + x));
                ++nrows;
            }
        }
        m |= (uint32_t)uqe[a * 5 + drop] << (3 + nrows);
        m |= (uint32_t)drop << (8 + 3 * nrows);
        spf[a * 5 + nrows] = pfs[a * 5 + drop];
        m |= (uint32_t)nrows;
        meta[a] = m;
        c->rows.h_row0[a + 1] = c->rows.h_row0[a] + nrows;
    }
    c->rows.R = c->rows.h_row0[L];
    c->rows.h_slot_meta = meta;
    c->rows.h_minor_w.assign((size_t)L, INT64_MAX);   // order key of the tile pruning (prep_block): rows with a table bin first, by weight
    for (int64_t a = 0; a < L; ++a)
        if ((meta[a] & 7u) == 1u && ((meta[a] >> 3) & 3u) == 3u && c->meta.h_r[(size_t)a] == 2.0) c->rows.h_minor_w[(size_t)a] = spf[a * 5];
    c->rows.h_span_bad.assign((size_t)L + 1, 0);
    for (int64_t a = 0; a < L; ++a) {
        const int n = (int)(meta[a] & 7u);
        const bool bad = n == 0 || ((n == 1 || n == 2) && (((meta[a] >> 3) & ((2u << n) - 1u)) != ((2u << n) - 1u)));
        c->rows.h_span_bad[(size_t)a + 1] = c->rows.h_span_bad[(size_t)a] + (bad ? 1 : 0);
    }
    const int64_t R = c->rows.R;
    lap("slot maps built on the host");
    if (int rc = c->rows.row0.reserve((size_t)(L + 1) * 4)) return rc;
    if (int rc = c->rows.slot_meta.reserve((size_t)L * 4)) return rc;
    if (int rc = c->rows.Mbits.reserve((size_t)(R + TILE) * c->KW * 8)) return rc;
    if (int rc = c->small.reserve((size_t)(R + 1) * 4)) return rc;
    LDW_HIP(hipMemcpyAsync(c->rows.row0.p, c->rows.h_row0.data(), (size_t)(L + 1) * 4, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(c->rows.slot_meta.p, meta.data(), (size_t)L * 4, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(c->rows.slot_pfix.p, spf.data(), (size_t)L * 40, hipMemcpyHostToDevice, c->stream));
    if (c->apx.apx_ok) {   // marginals of the approximate weights V' = a b 2^e by slot, in the accumulators' final unit 2^e_last (floor)
        if (int rc = slot_marginals(c, c->apx.h_vapx, c->apx.apx_e_last, c->rows.slot_papx, "approximate-weight marginals")) return rc;
    }
    // rows R .. R+TILE-1 stay zero: tile padding of the row lists points at row R
    LDW_HIP(hipMemsetAsync(c->rows.Mbits.as<uint64_t>() + (size_t)R * c->KW, 0, (size_t)TILE * c->KW * 8, c->stream));
    lap("approximate marginals");
    if (R > 0) {
        LDW_HIP(hipMemcpyAsync(c->small.p, rowinfo.data(), (size_t)R * 4, hipMemcpyHostToDevice, c->stream));
        LDW_REQUIRE(R < 2147483647LL, LDW_ERR_ARG, "too many indicator rows");
        if (int rc = fill_rows_bits(c, c->small.as<int32_t>(), R)) return rc;
    }
    if (int rc = c->rows.snp_sup.reserve((size_t)L * 32)) return rc;
    hipLaunchKernelGGL(k_snp_sup, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, c->stream, L, c->rows.slot_meta.as<uint32_t>(), c->rows.slot_pfix.as<int64_t>(),
                       c->meta.r.as<double>(), std::ldexp(1.0, -c->wts.frac_bits), c->wts.neff, c->meta.r_min, c->rows.snp_sup.as<double>());
    LDW_HIP(hipGetLastError());
    LDW_HIP(hipStreamSynchronize(c->stream));
    lap("bit rows + per-SNP bounds");
    c->rows_rebuilt();
    return LDW_OK;
}

}  // namespace ldw

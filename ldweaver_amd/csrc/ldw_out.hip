// The SNP alignment as text from the resident states: snpdat_to_fa (R/io_functions.R:363-417), generate_Links_SNPS_fasta (:432-460) and the
// snps.aln of write_output_for_gwes_explorer (R/createGWESExplorerOutput.R:23-76).
//
//   k_out_headers    : per record of the chunk the '>' name '\n' (FASTA) or the name (tsv), and the record's closing '\n'; one wave per record.
//   k_states_to_text : the body: a gather of the selected SNP rows of states [L][Npad] and a transpose through LDS, 64 SNPs x 64 sequences
//                      per tile (k_encode's tile, the other way round).  Reads run along the sequences of one SNP row, writes along the
//                      output row of one sequence; the tile is held as dwords with a row stride of 65, so neither phase meets a bank
//                      conflict.  States 0..4 print as A C G T N (the reference's one-hot rule: the N matrix stands for every other
//                      character, '-' included).
//
// Host driver (ldw_write_alignment): the sequences go out in chunks of whole records of at most chunk_bytes each (a larger record is a chunk
// of its own).  Both kernels and the D2H copy of chunk i run on the context's stream into one of two pinned buffers while the calling thread
// write()s chunk i - 1 from the other one; host memory stays at 2 x the largest chunk.  ldw_host_trim gives the pinned buffers back.
// Every offset is int64 and the grids are bounded by the chunk (grid-stride loops), not by L x N.  All global writes are plain C++ stores.
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "ldw_internal.h"

using namespace ldw;

namespace {

constexpr int OUT_TILE = 64;
constexpr int64_t OUT_DEFAULT_CHUNK = (int64_t)64 << 20;
constexpr int64_t OUT_MAX_BLOCKS = 8192;

__device__ __forceinline__ char state_char(uint32_t v) {
    return v < 4 ? (char)((0x54474341u >> (8 * v)) & 0xFFu) : 'N';   // "ACGT", then N
}

// Fmt 0: '>' name '\n' body '\n'.  Fmt 1: name body '\n'.  rec_off[0 .. ns]: absolute offsets of the chunk's records (the image starts at
// rec_off[0]); name_off[0 .. N]: offsets of the sequences' names in the blob (each followed by one separator byte).
template <int Fmt>
__global__ __launch_bounds__(256) void k_out_headers(const char *__restrict__ names, const int64_t *__restrict__ name_off, int64_t s0, int64_t ns,
                                                     const int64_t *__restrict__ rec_off, char *__restrict__ img) {
    const int lane = threadIdx.x & 63;
    const int64_t base = rec_off[0];
    for (int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < ns; q += (int64_t)gridDim.x * 4) {
        const int64_t nb = name_off[s0 + q], nl = name_off[s0 + q + 1] - nb - 1;
        char *rec = img + (rec_off[q] - base);
        char *dst = rec + (Fmt == 0 ? 1 : 0);
        for (int64_t b = lane; b < nl; b += 64) dst[b] = names[nb + b];
        if (lane == 0) {
            if (Fmt == 0) {
                rec[0] = '>';
                dst[nl] = '\n';
            }
            img[rec_off[q + 1] - base - 1] = '\n';
        }
    }
}

// tile t = (sequence tile) * ktiles + (SNP tile); the body of record q ends one byte before the record does
template <int Fmt>
__global__ __launch_bounds__(256) void k_states_to_text(const uint8_t *__restrict__ states, int64_t Npad, const int32_t *__restrict__ idx, int64_t k,
                                                        int64_t s0, int64_t ns, const int64_t *__restrict__ rec_off, char *__restrict__ img,
                                                        int64_t ktiles, int64_t ntiles) {
    __shared__ uint32_t tile[OUT_TILE][OUT_TILE + 1];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;   // 256 threads: 64 x 4
    const int64_t base = rec_off[0];
    const int64_t body_len = Fmt == 0 ? k : 2 * k;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t p0 = (t % ktiles) * OUT_TILE, q0 = (t / ktiles) * OUT_TILE;
        for (int i = ty; i < OUT_TILE; i += 4) {   // i: SNP within the tile, tx: sequence
            const int64_t p = p0 + i, q = q0 + tx;
            uint32_t v = 4;
            if (p < k && q < ns) v = states[(int64_t)idx[p] * Npad + s0 + q];
            tile[i][tx] = v;
        }
        __syncthreads();
        for (int i = ty; i < OUT_TILE; i += 4) {   // i: sequence within the tile, tx: SNP
            const int64_t q = q0 + i, p = p0 + tx;
            if (q < ns && p < k) {
                char *body = img + (rec_off[q + 1] - base - 1 - body_len);
                const char ch = state_char(tile[tx][i]);
                if (Fmt == 0) {
                    body[p] = ch;
                } else {
                    body[2 * p] = '\t';
                    body[2 * p + 1] = ch;
                }
            }
        }
        __syncthreads();
    }
}

// per context: the staging of the writer (made on first use, kept for the next call; ldw_host_trim / ldw_ctx_destroy give it back)
struct OutState {
    PinnedPair pin;
    DevBuf img, rec_off, name_off, names, idx;
    Event ev[2][3];   // per pinned buffer: before the kernels, after them, after the copy
};

OutState *out_state(ldw_ctx *c) {
    if (!c->out) c->out = new OutState();
    return static_cast<OutState *>(c->out);
}

int make_events(OutState *o) {
    for (auto &row : o->ev)
        for (auto &e : row)
            LDW_HIP(e.ensure());
    return LDW_OK;
}

int write_all(int fd, const char *p, size_t n, const char *path) {
    while (n > 0) {
        const ssize_t w = write(fd, p, n);
        if (w < 0) {
            if (errno == EINTR) continue;
            set_error("short write to %s: %s", path, strerror(errno));
            return LDW_ERR_ARG;
        }
        p += w;
        n -= (size_t)w;
    }
    return LDW_OK;
}

}  // namespace

namespace ldw {
void out_release(ldw_ctx *c) { release_state<OutState>(c, c->out); }

int64_t out_trim(ldw_ctx *c) {
    auto *o = static_cast<OutState *>(c->out);
    if (!o) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    const int64_t n = o->pin.release() + (int64_t)o->img.cap;
    o->img.release();
    return n;
}
}  // namespace ldw

extern "C" {

int ldw_write_alignment(ldw_ctx *c, const char *path, int append, int format, const int32_t *snp_idx, int64_t k, const char *names,
                        int64_t names_bytes, int64_t chunk_bytes, int64_t *bytes_out) {
    if (bytes_out) *bytes_out = 0;
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(ldw::have_alignment(c) && c->states.p, LDW_ERR_STATE, "ldw_write_alignment: no alignment resident");
    LDW_REQUIRE(path != nullptr, LDW_ERR_ARG, "ldw_write_alignment: null path");
    LDW_REQUIRE(format == 0 || format == 1, LDW_ERR_ARG, "ldw_write_alignment: format %d (0 FASTA, 1 tsv body)", format);
    LDW_REQUIRE(k >= 1 && snp_idx != nullptr, LDW_ERR_ARG, "ldw_write_alignment: k = %lld SNPs (at least 1)", (long long)k);
    for (int64_t i = 0; i < k; ++i)
        LDW_REQUIRE(snp_idx[i] >= 0 && snp_idx[i] < c->L, LDW_ERR_ARG, "ldw_write_alignment: snp_idx[%lld] = %d outside [0, %lld)", (long long)i,
                    snp_idx[i], (long long)c->L);
    LDW_REQUIRE(names != nullptr && names_bytes > 0, LDW_ERR_ARG, "ldw_write_alignment: no sequence names");
    // the names: NUL-separated, one per sequence (a last one without its NUL is accepted)
    const int64_t N = c->N;
    std::vector<int64_t> name_off;
    name_off.reserve((size_t)N + 1);
    name_off.push_back(0);
    for (int64_t b = 0; b < names_bytes; ++b) {
        LDW_REQUIRE(names[b] != '\n', LDW_ERR_ARG, "ldw_write_alignment: name %lld holds a newline", (long long)name_off.size() - 1);
        if (names[b] == '\0' || b + 1 == names_bytes) {
            LDW_REQUIRE((int64_t)name_off.size() <= N, LDW_ERR_ARG, "ldw_write_alignment: more than %lld names (one per sequence)", (long long)N);
            name_off.push_back(names[b] == '\0' ? b + 1 : b + 2);
        }
    }
    LDW_REQUIRE((int64_t)name_off.size() == N + 1, LDW_ERR_ARG, "ldw_write_alignment: %lld names for %lld sequences",
                (long long)name_off.size() - 1, (long long)N);
    // record offsets of the whole image, and the chunks of whole records
    const int64_t fixed = format == 0 ? 3 + k : 1 + 2 * k;   // '>' '\n' '\n' + k, or k x ('\t' c) + '\n'
    std::vector<int64_t> rec_off((size_t)N + 1);
    rec_off[0] = 0;
    for (int64_t s = 0; s < N; ++s) rec_off[(size_t)s + 1] = rec_off[(size_t)s] + (name_off[(size_t)s + 1] - name_off[(size_t)s] - 1) + fixed;
    const int64_t budget = chunk_bytes > 0 ? chunk_bytes : OUT_DEFAULT_CHUNK;
    std::vector<int64_t> cuts{0};
    int64_t cap = 0;
    for (int64_t s = 0; s < N;) {
        int64_t e = s + 1;
        while (e < N && rec_off[(size_t)e + 1] - rec_off[(size_t)s] <= budget) ++e;
        cap = std::max(cap, rec_off[(size_t)e] - rec_off[(size_t)s]);
        cuts.push_back(e);
        s = e;
    }
    // the file (truncated or appended to) before any device work: an unwritable path is an argument error
    const int fd = open(path, O_WRONLY | O_CREAT | (append ? O_APPEND : O_TRUNC), 0666);
    LDW_REQUIRE(fd >= 0, LDW_ERR_ARG, "cannot open %s: %s", path, strerror(errno));
    const bool timing = getenv("LDW_HOST_TIMING") != nullptr;   // (read per call, unlike ldw::host_timing(): a caller may switch it on for one file)
    int rc = LDW_OK;
    OutState *o = out_state(c);
    do {
        if ((rc = make_events(o))) break;
        if ((rc = o->pin.reserve((size_t)cap, "ldw_write_alignment"))) break;
        if ((rc = o->img.reserve((size_t)cap))) break;
        if ((rc = o->rec_off.reserve((size_t)(N + 1) * 8))) break;
        if ((rc = o->name_off.reserve((size_t)(N + 1) * 8))) break;
        if ((rc = o->names.reserve((size_t)names_bytes))) break;
        if ((rc = o->idx.reserve((size_t)k * 4))) break;
        hipError_t e = hipMemcpyAsync(o->rec_off.p, rec_off.data(), (size_t)(N + 1) * 8, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(o->name_off.p, name_off.data(), (size_t)(N + 1) * 8, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(o->names.p, names, (size_t)names_bytes, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(o->idx.p, snp_idx, (size_t)k * 4, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) {
            rc = hip_fail(e, "ldw_write_alignment: upload", __FILE__, __LINE__);
            break;
        }
    } while (false);
    // the pipeline: chunk i's kernels and copy are queued, then chunk i - 1 (already copied) is written while they run
    const int64_t nchunks = (int64_t)cuts.size() - 1;
    const int64_t ktiles = (k + OUT_TILE - 1) / OUT_TILE;
    double t_kernel = 0, t_copy = 0, t_write = 0;
    int64_t total = 0;
    auto write_chunk = [&](int64_t i) -> int {
        const int b = (int)(i & 1);
        const hipError_t e = hipEventSynchronize(o->ev[b][2]);
        if (e != hipSuccess) return hip_fail(e, "ldw_write_alignment: chunk copy", __FILE__, __LINE__);
        if (timing) {
            float a = 0, d = 0;
            (void)hipEventElapsedTime(&a, o->ev[b][0], o->ev[b][1]);
            (void)hipEventElapsedTime(&d, o->ev[b][1], o->ev[b][2]);
            t_kernel += a;
            t_copy += d;
        }
        const int64_t bytes = rec_off[(size_t)cuts[(size_t)i + 1]] - rec_off[(size_t)cuts[(size_t)i]];
        const auto w0 = std::chrono::steady_clock::now();
        if (int r = write_all(fd, o->pin.b[b].as<char>(), (size_t)bytes, path)) return r;
        t_write += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
        total += bytes;
        return LDW_OK;
    };
    for (int64_t i = 0; i < nchunks && rc == LDW_OK; ++i) {
        const int b = (int)(i & 1);
        const int64_t s0 = cuts[(size_t)i], ns = cuts[(size_t)i + 1] - s0;
        const int64_t bytes = rec_off[(size_t)s0 + (size_t)ns] - rec_off[(size_t)s0];
        const int64_t *d_rec = o->rec_off.as<int64_t>() + s0;
        const int64_t ntiles = ktiles * ((ns + OUT_TILE - 1) / OUT_TILE);
        const dim3 gh((unsigned)std::min<int64_t>((ns + 3) / 4, OUT_MAX_BLOCKS)), gb((unsigned)std::min<int64_t>(ntiles, OUT_MAX_BLOCKS));
        hipError_t e = hipEventRecord(o->ev[b][0], c->stream);
        if (format == 0) {
            hipLaunchKernelGGL(k_out_headers<0>, gh, dim3(256), 0, c->stream, o->names.as<char>(), o->name_off.as<int64_t>(), s0, ns, d_rec, o->img.as<char>());
            hipLaunchKernelGGL(k_states_to_text<0>, gb, dim3(256), 0, c->stream, c->states.as<uint8_t>(), c->Npad, o->idx.as<int32_t>(), k, s0, ns, d_rec,
                               o->img.as<char>(), ktiles, ntiles);
        } else {
            hipLaunchKernelGGL(k_out_headers<1>, gh, dim3(256), 0, c->stream, o->names.as<char>(), o->name_off.as<int64_t>(), s0, ns, d_rec, o->img.as<char>());
            hipLaunchKernelGGL(k_states_to_text<1>, gb, dim3(256), 0, c->stream, c->states.as<uint8_t>(), c->Npad, o->idx.as<int32_t>(), k, s0, ns, d_rec,
                               o->img.as<char>(), ktiles, ntiles);
        }
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(o->ev[b][1], c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(o->pin.b[b], o->img.p, (size_t)bytes, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipEventRecord(o->ev[b][2], c->stream);
        if (e != hipSuccess) {
            rc = hip_fail(e, "ldw_write_alignment: chunk", __FILE__, __LINE__);
            break;
        }
        if (i > 0) rc = write_chunk(i - 1);
    }
    if (rc == LDW_OK && nchunks > 0) rc = write_chunk(nchunks - 1);
    (void)hipStreamSynchronize(c->stream);   // (on an error path too: no copy may still land in a pinned buffer)
    if (close(fd) != 0 && rc == LDW_OK) {
        set_error("closing %s: %s", path, strerror(errno));
        rc = LDW_ERR_ARG;
    }
    if (timing && rc == LDW_OK)
        fprintf(stderr, "[ldw] write_alignment: %lld chunks, %lld bytes; kernels %.3f ms, copies %.3f ms, write %.3f ms\n", (long long)nchunks,
                (long long)total, t_kernel, t_copy, t_write);
    if (bytes_out) *bytes_out = total;
    return rc;
}

}  // extern "C"

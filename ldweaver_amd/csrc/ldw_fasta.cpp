// The native FASTA feeder: a FASTA file (plain or gzip) streamed one record at a time into pinned chunks of rows, each chunk copied to the
// device and counted there while the next one is parsed (pass 1, ldw_fasta_scan), then the retained columns encoded into the context's
// alignment (pass 2, ldw_fasta_encode) from a 4-bit packed device copy of the states kept by pass 1, or by reading the file again.  Host
// memory is O(io buffer + 2 chunks + one record), whatever the size of the alignment; the reference reads the file twice with kseq
// (src/getACGTNsites.cpp:13-176 counts, :179-291 extracts).
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <sys/stat.h>
#include <vector>
#include <zlib.h>

#include "ldw_internal.h"
#include "ldw_fasta.h"

namespace ldw {

// ------------------------------------------------------------------------------------------------
// the reader (host only)
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int64_t IO_DEFAULT = (int64_t)4 << 20;           // bytes per gzread
constexpr int64_t CHUNK_BYTES = (int64_t)32 << 20;         // default rows per chunk: about this many bytes
constexpr int64_t KEEP_MAX = (int64_t)8 << 30;             // automatic keep_bytes: at most this, and a quarter of the free device memory
const char *const ERR_NONE = "File does not contain any sequences!";
inline bool is_space(unsigned char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }
}  // namespace

FastaReader::~FastaReader() {
    if (gz_) gzclose((gzFile)gz_);
}

int FastaReader::open(const char *path, int64_t io_bytes) {
    LDW_REQUIRE(path != nullptr, LDW_ERR_ARG, "ldw_fasta: path is null");
    LDW_REQUIRE(io_bytes >= 0 && io_bytes <= ((int64_t)1 << 30), LDW_ERR_ARG, "ldw_fasta: io_bytes = %lld outside 0 .. 2^30", (long long)io_bytes);
    path_ = path;
    errno = 0;
    gzFile f = gzopen(path, "rb");
    LDW_REQUIRE(f != nullptr, LDW_ERR_ARG, "ldw_fasta: cannot open %s: %s", path, errno ? strerror(errno) : "out of memory");
    gz_ = f;
    const int64_t io = io_bytes ? io_bytes : IO_DEFAULT;
    gzbuffer(f, (unsigned)std::max<int64_t>(std::min<int64_t>(io, IO_DEFAULT), 65536));   // zlib's own input buffer
    buf_.resize((size_t)io);
    return LDW_OK;
}

int FastaReader::refill() {
    if (eof_) return 0;
    const int n = gzread((gzFile)gz_, buf_.data(), (unsigned)buf_.size());
    if (n < 0) {
        int code = 0;
        const char *msg = gzerror((gzFile)gz_, &code);
        set_error("ldw_fasta: reading %s failed: %s", path_.c_str(), msg ? msg : "unknown error");
        return -1;
    }
    if (n == 0) {
        eof_ = true;
        return 0;
    }
    pos_ = 0;
    end_ = (size_t)n;
    return 1;
}

// at a '>' at the start of a line: the whole header line (it may span reads), its name = the first whitespace-delimited token after '>'
int FastaReader::read_header(std::string &name) {
    std::string line;
    for (;;) {
        if (pos_ == end_) {
            const int r = refill();
            if (r < 0) return r;
            if (r == 0) break;
        }
        const unsigned char *a = buf_.data() + pos_;
        const unsigned char *nl = (const unsigned char *)memchr(a, '\n', end_ - pos_);
        const unsigned char *b = nl ? nl : buf_.data() + end_;
        line.append((const char *)a, b - a);
        pos_ = b - buf_.data();
        if (nl) {
            ++pos_;
            break;
        }
    }
    line_start_ = true;
    size_t i = 1;
    while (i < line.size() && is_space((unsigned char)line[i])) ++i;
    size_t j = i;
    while (j < line.size() && !is_space((unsigned char)line[j])) ++j;
    name.assign(line, i, j - i);
    return 1;
}

int FastaReader::next(std::string &name, char *dst, int64_t cap, std::vector<char> *grow, int64_t *len) {
    if (!started_) {   // lines before the first header are skipped
        for (;;) {
            if (pos_ == end_) {
                const int r = refill();
                if (r <= 0) return r;
            }
            if (line_start_ && buf_[pos_] == '>') {
                const int r = read_header(pending_);
                if (r < 0) return r;
                started_ = true;
                break;
            }
            const unsigned char *a = buf_.data() + pos_;
            const unsigned char *nl = (const unsigned char *)memchr(a, '\n', end_ - pos_);
            line_start_ = nl != nullptr;
            pos_ = nl ? (size_t)(nl - buf_.data()) + 1 : end_;
        }
    }
    if (!started_ || done_last_) return 0;
    name.swap(pending_);
    pending_.clear();
    int64_t n = 0, pend_cr = 0;   // pend_cr: '\r' at the end of what has been seen of the current line (kept only if more of the line follows)
    auto put = [&](const unsigned char *p, int64_t k) {
        if (grow) grow->insert(grow->end(), p, p + k);
        else if (n < cap) memcpy(dst + n, p, (size_t)std::min(k, cap - n));
        n += k;
    };
    bool more = false;
    for (;;) {
        if (pos_ == end_) {
            const int r = refill();
            if (r < 0) return r;
            if (r == 0) break;
        }
        if (line_start_) {
            if (buf_[pos_] == '>') {
                const int r = read_header(pending_);
                if (r < 0) return r;
                more = true;
                break;
            }
            line_start_ = false;
            pend_cr = 0;
        }
        const unsigned char *a = buf_.data() + pos_;
        const unsigned char *nl = (const unsigned char *)memchr(a, '\n', end_ - pos_);
        const unsigned char *b = nl ? nl : buf_.data() + end_;
        const unsigned char *e = b;
        while (e > a && e[-1] == '\r') --e;
        if (e > a) {
            static const unsigned char cr = '\r';
            for (; pend_cr > 0; --pend_cr) put(&cr, 1);
            put(a, e - a);
        }
        pend_cr += b - e;
        if (nl) {
            pos_ = (size_t)(nl - buf_.data()) + 1;
            line_start_ = true;
        } else {
            pos_ = end_;
        }
    }
    done_last_ = !more;
    *len = n;
    ++nrec_;
    return 1;
}

int fasta_check_len(int64_t rec, int64_t len, int64_t L, const std::string &name) {
    LDW_REQUIRE(len == L, LDW_ERR_ARG, "ldw_fasta: sequences are of different lengths (record %lld, '%s', has %lld characters, the first has %lld)",
                (long long)rec + 1, name.c_str(), (long long)len, (long long)L);
    return LDW_OK;
}

int file_stamp(const char *path, FileStamp *out) {
    struct stat st;
    LDW_REQUIRE(path && stat(path, &st) == 0, LDW_ERR_ARG, "ldw_fasta: cannot open %s: %s", path ? path : "(null)", strerror(errno));
    out->size = (int64_t)st.st_size;
    out->mtime_ns = (int64_t)st.st_mtim.tv_sec * 1000000000 + st.st_mtim.tv_nsec;
    return LDW_OK;
}

// the rest of a file whose first record is empty: "different lengths" if any record has a sequence, else "no sequences"
static int empty_first(FastaReader &rd) {
    std::string nm;
    int64_t len = 0;
    for (int r; (r = rd.next(nm, nullptr, 0, nullptr, &len)) != 0;) {
        if (r < 0) return LDW_ERR_ARG;
        if (int rc = fasta_check_len(rd.records() - 1, len, 0, nm)) return rc;
    }
    set_error("ldw_fasta: %s", ERR_NONE);
    return LDW_ERR_ARG;
}

static int copy_names(const std::string &names, char *out, int64_t cap, int64_t *bytes, const char *who) {
    if (bytes) *bytes = (int64_t)names.size();
    if (!out) return LDW_OK;
    LDW_REQUIRE(cap >= (int64_t)names.size(), LDW_ERR_SIZE, "%s: the names need %lld bytes, names_cap is %lld", who, (long long)names.size(), (long long)cap);
    memcpy(out, names.data(), names.size());
    return LDW_OK;
}

// ------------------------------------------------------------------------------------------------
// the scan state of a context
// ------------------------------------------------------------------------------------------------
struct FastaScan {
    bool done = false;                 // a complete pass 1: what follows describes it
    std::string path, names;           // names: NUL-terminated, one per record
    FileStamp stamp;
    int64_t N = 0, L = 0, Lp = 0, chunk_rows = 0, io_bytes = 0;
    DevBuf counts;                     // int32 [Lp][5] (the first L columns are the file's)
    DevBuf packed;                     // uint8 [N][Lp / 2]: 4-bit states, while `kept`
    bool kept = false;
    PinnedPair pin;                    // pinned chunks [rows][Lp]
    DevBuf dchunk[2];                  // their device images
    Event ev[2];                       // recorded after the copy of a chunk out of pin[k] (and the kernel behind it)
    bool ev_live[2] = {false, false};
};

static FastaScan *scan_state(ldw_ctx *c) {
    if (!c->fasta) c->fasta = new FastaScan();
    return static_cast<FastaScan *>(c->fasta);
}

// the chunk ring goes: the pinned pair and its device images; bytes released
static int64_t free_chunks(FastaScan *f) {
    int64_t n = f->pin.release();
    for (int k = 0; k < 2; ++k) {
        n += (int64_t)f->dchunk[k].cap;
        f->dchunk[k].release();
        f->ev_live[k] = false;
    }
    return n;
}

void fasta_release(ldw_ctx *c) { release_state<FastaScan>(c, c->fasta); }

int64_t fasta_trim(ldw_ctx *c) {
    auto *f = static_cast<FastaScan *>(c->fasta);
    if (!f) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    return free_chunks(f);
}

// two pinned chunks of `bytes` each and their device images; events once
static int ensure_chunks(FastaScan *f, size_t bytes) {
    for (auto &e : f->ev) LDW_HIP(e.ensure(hipEventDisableTiming));
    if (int rc = f->pin.reserve(bytes, "ldw_fasta")) return rc;
    for (int k = 0; k < 2; ++k)
        if (int rc = f->dchunk[k].reserve(bytes)) return rc;
    return LDW_OK;
}

// the chunk ring: parse into pin[k] while the device copies and processes pin[k ^ 1]
static int wait_chunk(FastaScan *f, int k) {
    if (f->ev_live[k]) LDW_HIP(hipEventSynchronize(f->ev[k]));
    f->ev_live[k] = false;
    return LDW_OK;
}

static int upload_chunk(ldw_ctx *c, FastaScan *f, int k, int64_t rows) {
    LDW_HIP(hipMemcpyAsync(f->dchunk[k].p, f->pin.b[k], (size_t)(rows * f->Lp), hipMemcpyHostToDevice, c->stream));
    return LDW_OK;
}

static int chunk_done(ldw_ctx *c, FastaScan *f, int k) {
    LDW_HIP(hipEventRecord(f->ev[k], c->stream));
    f->ev_live[k] = true;
    return LDW_OK;
}

// the row r of pin[k]: its padding bytes L .. Lp are zeroed (the kernels read whole 16-byte groups)
static inline char *pin_row(FastaScan *f, int k, int64_t r) {
    char *row = f->pin.b[k].as<char>() + r * f->Lp;
    if (f->Lp > f->L) memset(row + f->L, 0, (size_t)(f->Lp - f->L));
    return row;
}

}  // namespace ldw

using namespace ldw;

extern "C" {

int ldw_fasta_probe(const char *path, int64_t io_bytes, int64_t *N, int64_t *L_total, char *names, int64_t names_cap, int64_t *names_bytes) {
    LDW_REQUIRE(path && N && L_total, LDW_ERR_ARG, "ldw_fasta_probe: null argument");
    FastaReader rd;
    if (int rc = rd.open(path, io_bytes)) return rc;
    std::string nm, all;
    int64_t L = -1, len = 0;
    for (int r; (r = rd.next(nm, nullptr, 0, nullptr, &len)) != 0;) {
        if (r < 0) return LDW_ERR_ARG;
        if (L < 0) {
            if (len == 0) return empty_first(rd);
            L = len;
        } else if (int rc = fasta_check_len(rd.records() - 1, len, L, nm)) {
            return rc;
        }
        all.append(nm);
        all.push_back('\0');
    }
    LDW_REQUIRE(L > 0, LDW_ERR_ARG, "ldw_fasta: %s", ERR_NONE);
    *N = rd.records();
    *L_total = L;
    return copy_names(all, names, names_cap, names_bytes, "ldw_fasta_probe");
}

int ldw_fasta_scan(ldw_ctx *c, const char *path, int64_t chunk_rows, int64_t io_bytes, int64_t keep_bytes, int64_t *N_out, int64_t *L_total_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(path && chunk_rows >= 0, LDW_ERR_ARG, "ldw_fasta_scan: bad argument");
    if (int rc = join_prepare(c)) return rc;
    FastaScan *f = scan_state(c);
    LDW_HIP(hipStreamSynchronize(c->stream));
    f->done = false;   // a new scan discards the last one
    f->kept = false;
    f->packed.release();
    f->names.clear();
    FileStamp stamp;
    if (int rc = file_stamp(path, &stamp)) return rc;
    FastaReader rd;
    if (int rc = rd.open(path, io_bytes)) return rc;
    std::vector<char> first;
    std::string nm;
    int64_t len = 0;
    {
        const int r = rd.next(nm, nullptr, 0, &first, &len);
        if (r < 0) return LDW_ERR_ARG;
        LDW_REQUIRE(r > 0, LDW_ERR_ARG, "ldw_fasta: %s", ERR_NONE);
        if (len == 0) return empty_first(rd);
    }
    const int64_t L = len, Lp = (L + 15) / 16 * 16;
    const int64_t rows = chunk_rows > 0 ? chunk_rows : std::max<int64_t>(1, CHUNK_BYTES / L);
    if (int rc = ensure_chunks(f, (size_t)(rows * Lp))) return rc;
    if (int rc = f->counts.reserve((size_t)Lp * 20)) return rc;
    LDW_HIP(hipMemsetAsync(f->counts.p, 0, (size_t)Lp * 20, c->stream));
    int64_t budget = keep_bytes;   // bytes the packed copy may take
    if (keep_bytes < 0) {
        size_t fr = 0, tot = 0;
        LDW_HIP(hipMemGetInfo(&fr, &tot));
        budget = std::min<int64_t>(KEEP_MAX, (int64_t)(fr / 4));
    }
    bool pack = budget > 0;
    f->L = L;
    f->Lp = Lp;
    // the ring; every error below drains the stream first (the copies read the pinned chunks)
    auto fail = [&](int rc) {
        (void)hipStreamSynchronize(c->stream);
        f->ev_live[0] = f->ev_live[1] = false;
        f->packed.release();
        return rc;
    };
    int k = 0;
    if (int rc = wait_chunk(f, 0)) return fail(rc);
    memcpy(pin_row(f, 0, 0), first.data(), (size_t)L);
    std::vector<char>().swap(first);
    f->names.append(nm).push_back('\0');
    int64_t s0 = 0, r = 1;
    bool eof = false;
    for (;;) {
        while (r < rows) {
            const int rr = rd.next(nm, pin_row(f, k, r), L, nullptr, &len);
            if (rr < 0) return fail(LDW_ERR_ARG);
            if (rr == 0) {
                eof = true;
                break;
            }
            if (int rc = fasta_check_len(rd.records() - 1, len, L, nm)) return fail(rc);
            f->names.append(nm).push_back('\0');
            ++r;
        }
        if (r > 0) {
            uint8_t *pk = nullptr;
            if (pack) {
                const int64_t need = (s0 + r) * (Lp / 2);
                if (need > budget) {   // the packed copy would not fit: pass 2 reads the file again
                    pack = false;
                    LDW_HIP(hipStreamSynchronize(c->stream));
                    f->packed.release();
                } else {
                    // growing the copy drains the stream: the first reservation is the row count a plain file of this size can hold (a gz
                    // file's grows from there), and every growth at least doubles it
                    int64_t want = std::max<int64_t>(need, 2 * (int64_t)f->packed.cap);
                    if (!f->packed.p) want = std::max<int64_t>(need, (stamp.size / L + 1) * (Lp / 2));
                    want = std::min<int64_t>(want, std::max<int64_t>(need, budget));
                    if ((size_t)need > f->packed.cap)
                        if (int rc = f->packed.reserve_keep((size_t)want, (size_t)(s0 * (Lp / 2)), c->stream)) return fail(rc);
                    pk = f->packed.as<uint8_t>() + s0 * (Lp / 2);
                }
            }
            if (int rc = upload_chunk(c, f, k, r)) return fail(rc);
            if (int rc = launch_fasta_count_pack(f->dchunk[k].as<uint8_t>(), r, L, Lp, f->counts.as<int32_t>(), pk, c->stream)) return fail(rc);
            if (int rc = chunk_done(c, f, k)) return fail(rc);
            s0 += r;
        }
        if (eof) break;
        k ^= 1;
        if (int rc = wait_chunk(f, k)) return fail(rc);
        r = 0;
    }
    LDW_HIP(hipStreamSynchronize(c->stream));
    f->ev_live[0] = f->ev_live[1] = false;
    f->path = path;
    f->stamp = stamp;
    f->N = s0;
    f->chunk_rows = rows;
    f->io_bytes = io_bytes;
    f->kept = pack;
    f->done = true;
    if (N_out) *N_out = s0;
    if (L_total_out) *L_total_out = L;
    return LDW_OK;
}

int ldw_fasta_counts(ldw_ctx *c, int32_t *allele_counts_out) {
    if (int rc = check_gpu(c)) return rc;
    auto *f = static_cast<FastaScan *>(c->fasta);
    LDW_REQUIRE(f && f->done, LDW_ERR_STATE, "ldw_fasta_counts: no FASTA scan on this context");
    LDW_REQUIRE(allele_counts_out, LDW_ERR_ARG, "ldw_fasta_counts: null argument");
    LDW_HIP(hipMemcpyAsync(allele_counts_out, f->counts.p, (size_t)f->L * 20, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

int ldw_fasta_names(ldw_ctx *c, char *names, int64_t cap, int64_t *names_bytes) {
    LDW_REQUIRE(c, LDW_ERR_ARG, "null context");
    auto *f = static_cast<FastaScan *>(c->fasta);
    LDW_REQUIRE(f && f->done, LDW_ERR_STATE, "ldw_fasta_names: no FASTA scan on this context");
    return copy_names(f->names, names, cap, names_bytes, "ldw_fasta_names");
}

int ldw_fasta_encode(ldw_ctx *c, const int32_t *pos, int64_t n_pos, int32_t *acgtn_table_out) {
    if (int rc = check_gpu(c)) return rc;
    auto *f = static_cast<FastaScan *>(c->fasta);
    LDW_REQUIRE(f && f->done, LDW_ERR_STATE, "ldw_fasta_encode: no FASTA scan on this context");
    LDW_REQUIRE(pos && n_pos > 0, LDW_ERR_ARG, "ldw_fasta_encode: bad argument");
    for (int64_t i = 0; i < n_pos; ++i)
        LDW_REQUIRE(pos[i] >= 1 && pos[i] <= f->L, LDW_ERR_ARG, "ldw_fasta_encode: pos[%lld]=%d outside 1..%lld", (long long)i, pos[i], (long long)f->L);
    const int64_t N = f->N, L = f->L, Lp = f->Lp;
    if (!f->kept) {
        FileStamp now;
        if (file_stamp(f->path.c_str(), &now) != LDW_OK || !(now == f->stamp)) {
            set_error("ldw_fasta_encode: %s changed since ldw_fasta_scan (size or modification time)", f->path.c_str());
            return LDW_ERR_STATE;
        }
    }
    if (int rc = set_dims(c, n_pos, N)) return rc;
    if (int rc = c->scratch.reserve((size_t)n_pos * 4)) return rc;
    int32_t *d_pos = c->scratch.as<int32_t>();
    LDW_HIP(hipMemcpyAsync(d_pos, pos, (size_t)n_pos * 4, hipMemcpyHostToDevice, c->stream));
    uint8_t *states = c->states.as<uint8_t>();
    auto fail = [&](int rc) {
        (void)hipStreamSynchronize(c->stream);
        f->ev_live[0] = f->ev_live[1] = false;
        c->L = 0;   // no alignment resident
        return rc;
    };
    if (f->kept) {   // from the packed copy: one launch over all sequences, then the copy goes
        if (int rc = launch_fasta_encode_rows(true, f->packed.as<uint8_t>(), Lp / 2, 0, 0, c->Npad, N, d_pos, n_pos, states, c->Npad, c->stream)) return fail(rc);
        LDW_HIP(hipStreamSynchronize(c->stream));
        f->packed.release();
        f->kept = false;
    } else {         // read the file again, chunk by chunk
        FastaReader rd;
        if (int rc = rd.open(f->path.c_str(), f->io_bytes)) return fail(rc);
        const int64_t rows = f->chunk_rows;
        if (int rc = ensure_chunks(f, (size_t)(rows * Lp))) return fail(rc);
        std::string nm;
        int64_t len = 0, s0 = 0;
        for (int k = 0; s0 < N; k ^= 1) {
            if (int rc = wait_chunk(f, k)) return fail(rc);
            const int64_t want = std::min(rows, N - s0);
            for (int64_t r = 0; r < want; ++r) {
                const int rr = rd.next(nm, pin_row(f, k, r), L, nullptr, &len);
                if (rr < 0) return fail(LDW_ERR_ARG);
                LDW_REQUIRE(rr > 0 && len == L, fail(LDW_ERR_STATE), "ldw_fasta_encode: %s no longer has the shape the scan read (%lld x %lld)",
                            f->path.c_str(), (long long)N, (long long)L);
            }
            if (int rc = upload_chunk(c, f, k, want)) return fail(rc);
            const int64_t s_end = s0 + want == N ? c->Npad : s0 + want;
            if (int rc = launch_fasta_encode_rows(false, f->dchunk[k].as<uint8_t>(), Lp, s0, s0, s_end, N, d_pos, n_pos, states, c->Npad, c->stream))
                return fail(rc);
            if (int rc = chunk_done(c, f, k)) return fail(rc);
            s0 += want;
        }
        const int rr = rd.next(nm, nullptr, 0, nullptr, &len);
        LDW_REQUIRE(rr == 0, fail(LDW_ERR_STATE), "ldw_fasta_encode: %s no longer has the shape the scan read (%lld x %lld)", f->path.c_str(),
                    (long long)N, (long long)L);
        LDW_HIP(hipStreamSynchronize(c->stream));
        f->ev_live[0] = f->ev_live[1] = false;
    }
    if (acgtn_table_out) return ldw_state_counts(c, acgtn_table_out);
    return LDW_OK;
}

}  // extern "C"

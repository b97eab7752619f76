// The native FASTA feeder: the streaming reader and the scan state (ldw_fasta.cpp), the kernels' launchers (ldw_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

struct ldw_ctx;

namespace ldw {

// One pass over a FASTA file, plain or gzip (zlib's gzread reads both, multi-member gz included), one record at a time in O(io buffer)
// memory.  Record rules (those of snpdat.read_fasta, except for the lines before the first header, which are skipped as the reference's
// reader skips them): a header line starts with '>', its name is the first whitespace-delimited token after it ("" if none); every other
// line is sequence; trailing '\r' / '\n' are stripped, blank lines skipped, every other byte (spaces included) kept.
class FastaReader {
public:
    FastaReader() = default;
    ~FastaReader();
    FastaReader(const FastaReader &) = delete;
    FastaReader &operator=(const FastaReader &) = delete;

    int open(const char *path, int64_t io_bytes);   // LDW_OK, or an error status with ldw_last_error() set
    // The next record: its name into `name`, its sequence bytes into dst[0 .. cap) — bytes past cap are counted but not stored — or, with
    // grow non-null, appended to *grow.  *len receives the record's full length.  Returns 1 for a record, 0 at the end, < 0 on a read error.
    int next(std::string &name, char *dst, int64_t cap, std::vector<char> *grow, int64_t *len);
    int64_t records() const { return nrec_; }

private:
    int refill();   // 1: bytes available, 0: end of file, < 0: read error
    int read_header(std::string &name);
    void *gz_ = nullptr;
    std::vector<unsigned char> buf_;
    size_t pos_ = 0, end_ = 0;
    bool eof_ = false, started_ = false, line_start_ = true;
    bool done_last_ = false;   // the last record has been returned
    std::string pending_;   // name of the record whose header has been read
    int64_t nrec_ = 0;
    std::string path_;
};

// ldw_fasta_scan's whole-file shape check for one record: "sequences are of different lengths" (ldw_last_error) unless len == L
int fasta_check_len(int64_t rec, int64_t len, int64_t L, const std::string &name);

// identity of the file a scan read (pass 2 re-reads it only if it is unchanged)
struct FileStamp {
    int64_t size = -1, mtime_ns = -1;
    bool operator==(const FileStamp &o) const { return size == o.size && mtime_ns == o.mtime_ns; }
};
int file_stamp(const char *path, FileStamp *out);

void fasta_release(ldw_ctx *ctx);       // the scan state of the context (pinned buffers, packed copy, counts); ldw_ctx_destroy
int64_t fasta_trim(ldw_ctx *ctx);       // the pinned chunk buffers and their device images only (ldw_host_trim); bytes released

// ldw_api.hip, beside k_encode; asynchronous on `s`.
// k_fasta_count_pack: a chunk of `rows` sequences, chunk[r * Lp + j] (Lp = L rounded up to 16), adds its per-column A/C/G/T/other counts
// into counts [Lp][5] (the columns from L on count the chunk's zero padding); with packed non-null it also writes the chunk's states, 4 bits each, into packed[r * Lp / 2 + j / 2] (low nibble: even j).
int launch_fasta_count_pack(const uint8_t *chunk, int64_t rows, int64_t L, int64_t Lp, int32_t *counts, uint8_t *packed, hipStream_t s);
// k_fasta_encode_rows: states[p][s] for sequences s0 <= s < s_end (< Npad; 255 from N on) of the retained 1-based columns pos[n_pos], read from
// src (raw chars when !packed, 4-bit states when packed) whose row s - src_s0 starts at byte (s - src_s0) * stride
int launch_fasta_encode_rows(bool packed, const uint8_t *src, int64_t stride, int64_t src_s0, int64_t s0, int64_t s_end, int64_t N,
                             const int32_t *pos, int64_t n_pos, uint8_t *states, int64_t Npad, hipStream_t s);

}  // namespace ldw

// The native reader of numeric link tables (include/ldweaver_amd.h 13): the host side (ldw_links_read_host.cpp: probe, chunk feeder, line
// look-up, slow-cell conversion) and what the context's other translation units need of the device side (ldw_links_read.hip).
#pragma once
#include <stdint.h>
#include <string>

struct ldw_ctx;

namespace ldw {

constexpr int64_t TSV_LINE_MAX = 1 << 20;        // bytes of one line before its '\n': a longer line is refused
constexpr int64_t TSV_DEFAULT_CHUNK = 64 << 20;
constexpr int64_t TSV_FRONT = 16;                // '\n' bytes in front of a chunk's data: byte -1 of the first line, and the data stays 16-byte aligned
constexpr int64_t TSV_TAIL = 48;                 // '\n' bytes behind it: what the kernels may read past the last line (a 16-byte load, a 3-byte token look-ahead)
constexpr int TSV_MAX_COLS = 16;

// One pass over a text file, plain or gzip (zlib's gzread reads both), in chunks cut at their last '\n'.
class TsvFeeder {
public:
    TsvFeeder() = default;
    ~TsvFeeder() { close(); }
    TsvFeeder(const TsvFeeder &) = delete;
    TsvFeeder &operator=(const TsvFeeder &) = delete;
    int open(const char *path);   // LDW_OK, or LDW_ERR_ARG "cannot open"
    void close();
    // data[0 .. carry) holds the unfinished line the last chunk ended with.  Reads up to chunk_bytes more at a time (cap >= chunk_bytes + TSV_LINE_MAX + 1)
    // until the buffer holds a '\n' or the file ends (a last line without one gets it).  *cut = bytes of whole lines (0 at the end of the file), *total = bytes
    // in the buffer: data[*cut .. *total) is the next carry.  LDW_ERR_ARG for a line over TSV_LINE_MAX (*cut = -1: the caller names the line) or a read error.
    int fill(char *data, int64_t carry, int64_t chunk_bytes, int64_t cap, int64_t *cut, int64_t *total);
    bool gzip() const { return gzip_; }
    double read_ms = 0;           // host time spent inside gzread

private:
    void *gz_ = nullptr;
    bool eof_ = false, gzip_ = false;
    std::string path_;
};

// (error paths only: the file is read again)  1-based physical line of the row-th (0-based) non-empty line; of the line that holds byte `off`
int tsv_line_of_row(const char *path, int64_t row, int64_t *line_out);
int tsv_line_of_offset(const char *path, int64_t off, int64_t *line_out);
// correctly rounded double of the decimal text at p (strtod_l in the "C" locale); the text ends at the first byte strtod does not take
double tsv_strtod(const char *p);

// The header line text[0 .. len) (no '\n'; a '\r' at its end is dropped) of a tab-separated table: col_out[k] = 0-based column named names[k], *ncols_out = its
// fields.  LDW_ERR_ARG, the message naming path, `line` and a 1-based column: a name that is missing (column = fields + 1) or there twice (column = the second
// one), more than max_cols fields.
int tsv_header_columns(const char *path, int64_t line, const char *text, int64_t len, const char *const *names, int n_names, int max_cols, int32_t *col_out,
                       int32_t *ncols_out);
// ldw_links_read.hip, for another pass over a text file (ldw_links_grep.hip).  The reader's two pinned chunk buffers (their TSV_FRONT bytes set to '\n') and
// the device image, with room for chunks of `chunk` bytes: *cap_out = data bytes a buffer holds (TsvFeeder::fill's cap).  They are the reader's own: a
// pass that uses them must finish before the next ldw_tsv_read starts (both run on the context's stream, from the caller's thread).
int tsv_chunk_buffers(ldw_ctx *ctx, int64_t chunk, void *pin[2], uint8_t **d_img, int64_t *cap_out);
// The non-empty lines of the `cut` bytes at d_buf (device; '\n' in front and behind as TSV_FRONT / TSV_TAIL have it), queued on the context's stream:
// k_tsv_count and the exclusive sums, *d_total = device address of the line count; then, the count known, k_tsv_starts: (*d_starts)[k] = first byte of line k.
int tsv_rows_count(ldw_ctx *ctx, const uint8_t *d_buf, int64_t cut, const uint32_t **d_total);
int tsv_rows_starts(ldw_ctx *ctx, const uint8_t *d_buf, int64_t cut, uint32_t nrows, const uint32_t **d_starts);

void tsv_release(ldw_ctx *ctx);      // ldw_links_read.hip: the reader's state (ldw_ctx_destroy)
int64_t tsv_trim(ldw_ctx *ctx);      // ... its pinned chunk buffers and the chunk's device image only (ldw_host_trim); bytes released
void grep_release(ldw_ctx *ctx);     // ldw_links_grep.hip: the search's state (ldw_ctx_destroy)
int64_t grep_trim(ldw_ctx *ctx);     // ... its device records and the host copy of the last result (ldw_host_trim); bytes released

}  // namespace ldw

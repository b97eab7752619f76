// The native reader of numeric link tables (include/ldweaver_amd.h 13): the host side (ldw_links_read_host.cpp: probe, chunk feeder, line
// look-up, slow-cell conversion), the chunk pass both text-file entries run on, and what the context's other translation units need of the device
// side (ldw_links_read.hip).
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

// reasons a row is refused (the low byte of the kernels' bad-row key)
enum { BAD_CELL = 1, BAD_MISSING = 2, BAD_EXTRA = 3, BAD_LONG = 4 };

// One pass over a text file in chunks of whole lines, through two buffers and one device image laid out  TSV_FRONT '\n' | data | TSV_TAIL '\n'
// (ldw_tsv_read, ldw_links_grep).  A user's loop:
//     open(); attach();
//     for (; more(); advance()) {
//         [finish the chunk before this one: its text lies in buffer 1 - buffer() until begin() moves the carried line there]
//         text = begin(); queue();
//         prefetch() and wait(&rows), in the order the user overlaps them; its own kernels over d_text() / starts();
//     }
//     refusal, if none of its own came first: feeder_refusal()
// The host half (ldw_links_read_host.cpp) needs no device: use() takes any two buffers.  The stream half (ldw_links_read.hip) borrows the reader's pinned
// pair, image and line-kernel work space, which are the context's: a pass ends before the next begins (both run on the context's stream, from the
// caller's thread), and its destructor waits for the stream, so no copy still reads a pinned buffer on whichever path the user leaves.
class TsvPass {
public:
    TsvPass(const char *who, const char *path) : who_(who), path_(path) {}
    ~TsvPass() {
        if (ctx_) drain();
    }
    TsvPass(const TsvPass &) = delete;
    TsvPass &operator=(const TsvPass &) = delete;

    // ---- host half
    int open(int64_t chunk_bytes);   // chunk_bytes in 0..2^30 (0: TSV_DEFAULT_CHUNK), then the file
    int64_t buffer_bytes() const { return TSV_FRONT + cap_ + TSV_TAIL; }   // of each of the two buffers (after open)
    void use(void *b0, void *b1);    // the buffers: their TSV_FRONT bytes become '\n', the first chunk is read (a refusal of it waits for feeder_refusal)
    bool more() const { return cut_ > 0; }
    int buffer() const { return (int)(k_ & 1); }                                        // the buffer of the chunk more() announces
    const char *text(int b) const { return static_cast<const char *>(buf_[b]) + TSV_FRONT; }
    int64_t cut() const { return cut_; }                                                // its bytes: whole lines, the last '\n' included
    char *begin();                   // moves the line the chunk ends with into the other buffer, pads this one's tail with '\n'; the chunk's text
    void prefetch();                 // reads the next chunk into the other buffer, behind the carried line; a refusal is kept for feeder_refusal
    void advance();                  // the prefetched chunk becomes the current one (none after the last, or after a refusal)
    // LDW_OK, or what the feeder refused: a line over TSV_LINE_MAX as "line N, column 1: the line is longer than ..." (the error is set)
    int feeder_refusal() const;
    int refuse_row(int64_t row, uint32_t col, uint32_t reason, int ncols) const;   // row: 0-based among the non-empty lines; reason: BAD_*; LDW_ERR_ARG
    bool gzip() const { return feed_.gzip(); }
    double read_ms() const { return feed_.read_ms; }
    int64_t consumed = 0, nchunks = 0;   // bytes and chunks queued so far
    double copy_ms = 0, line_ms = 0;     // device time of the chunks waited for: the copies; k_tsv_count and the sums

    // ---- stream half
    int attach(ldw_ctx *ctx);        // the context's buffers, grown to this pass's chunk size, then use()
    const uint8_t *d_text() const { return d_text_; }    // the image's data: device twin of text(buffer())
    // copies the chunk and counts its non-empty lines on the context's stream (k_tsv_count, the exclusive sums, the count's way back); does not wait
    int queue();
    const uint32_t *d_rows() const { return d_rows_; }   // device address of that count (valid behind queue() on the stream)
    int wait(uint32_t *rows);        // ... waits for it
    int starts(uint32_t rows, const uint32_t **d_starts);   // queues k_tsv_starts: (*d_starts)[k] = first byte of line k, from d_text()

private:
    void drain();
    const char *who_, *path_;
    TsvFeeder feed_;
    int64_t chunk_ = 0, cap_ = 0;    // bytes read at a time; data bytes of a buffer: a carried line and a chunk
    void *buf_[2] = {nullptr, nullptr};
    int64_t k_ = 0, cut_ = 0, total_ = 0, next_cut_ = 0, next_total_ = 0;
    int fill_rc_ = 0;
    std::string fill_err_;
    ldw_ctx *ctx_ = nullptr;
    const uint8_t *d_text_ = nullptr;
    const uint32_t *d_rows_ = nullptr;
};

void tsv_release(ldw_ctx *ctx);      // ldw_links_read.hip: the reader's state (ldw_ctx_destroy)
int64_t tsv_trim(ldw_ctx *ctx);      // ... its pinned chunk buffers and the chunk's device image only (ldw_host_trim); bytes released
void grep_release(ldw_ctx *ctx);     // ldw_links_grep.hip: the search's state (ldw_ctx_destroy)
int64_t grep_trim(ldw_ctx *ctx);     // ... its device records and the host copy of the last result (ldw_host_trim); bytes released

}  // namespace ldw

// Host side of the native reader of numeric link tables (include/ldweaver_amd.h 13): ldw_tsv_probe, the chunk feeder, the host half of
// the chunk pass, the physical line of a row (error paths) and the conversion of the cells the device leaves to the host.
#include <errno.h>
#include <locale.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "ldw_internal.h"
#include "ldw_links_read.h"

namespace ldw {

int TsvFeeder::open(const char *path) {
    close();
    errno = 0;
    gzFile f = gzopen(path, "rb");
    LDW_REQUIRE(f != nullptr, LDW_ERR_ARG, "ldw_tsv: cannot open %s: %s", path, errno ? strerror(errno) : "out of memory");
    gzbuffer(f, 1u << 20);
    gz_ = f;
    gzip_ = gzdirect(f) == 0;
    eof_ = false;
    path_ = path;
    read_ms = 0;
    return LDW_OK;
}

void TsvFeeder::close() {
    if (gz_) gzclose(static_cast<gzFile>(gz_));
    gz_ = nullptr;
}

int TsvFeeder::fill(char *data, int64_t carry, int64_t chunk_bytes, int64_t cap, int64_t *cut, int64_t *total) {
    int64_t size = carry;
    *cut = 0;
    *total = size;
    for (;;) {
        if (eof_) {   // what is left is the last line, without its newline
            if (size > 0) {
                if (size > TSV_LINE_MAX) {
                    *cut = -1;
                    set_error("ldw_tsv_read: %s: a line is longer than %lld bytes", path_.c_str(), (long long)TSV_LINE_MAX);
                    return LDW_ERR_ARG;
                }
                data[size++] = '\n';
            }
            *cut = *total = size;
            return LDW_OK;
        }
        const int64_t want = std::min<int64_t>(std::min<int64_t>(chunk_bytes, cap - 1 - size), 1 << 30);
        const auto t0 = std::chrono::steady_clock::now();
        const int got = gzread(static_cast<gzFile>(gz_), data + size, (unsigned)want);
        read_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (got < 0) {
            int errnum = 0;
            const char *msg = gzerror(static_cast<gzFile>(gz_), &errnum);
            set_error("ldw_tsv_read: reading %s: %s", path_.c_str(), errnum == Z_ERRNO ? strerror(errno) : msg);
            return LDW_ERR_ARG;
        }
        if (got < want) eof_ = true;
        // the carry holds no newline, so the last newline of the buffer, if any, is among the new bytes
        const void *nl = got > 0 ? memrchr(data + size, '\n', (size_t)got) : nullptr;
        size += got;
        *total = size;
        if (nl) {
            *cut = (int64_t)(static_cast<const char *>(nl) - data) + 1;
            return LDW_OK;
        }
        if (size > TSV_LINE_MAX) {
            *cut = -1;
            set_error("ldw_tsv_read: %s: a line is longer than %lld bytes", path_.c_str(), (long long)TSV_LINE_MAX);
            return LDW_ERR_ARG;
        }
    }
}

// ---- TsvPass, the host half -----------------------------------------------------------------------------------------------------------------------

int TsvPass::open(int64_t chunk_bytes) {
    LDW_REQUIRE(chunk_bytes >= 0 && chunk_bytes <= ((int64_t)1 << 30), LDW_ERR_ARG, "%s: chunk_bytes = %lld outside 0..2^30 (0: 64 MiB)", who_, (long long)chunk_bytes);
    chunk_ = chunk_bytes > 0 ? chunk_bytes : TSV_DEFAULT_CHUNK;
    cap_ = chunk_ + TSV_LINE_MAX + 64;
    return feed_.open(path_);
}

void TsvPass::use(void *b0, void *b1) {
    buf_[0] = b0;
    buf_[1] = b1;
    for (void *b : buf_) memset(b, '\n', (size_t)TSV_FRONT);
    k_ = -1;             // the first chunk is "prefetched" into buffer 0 behind an empty carry
    total_ = cut_ = 0;
    prefetch();
    advance();
}

char *TsvPass::begin() {
    const int b = buffer();
    char *data = static_cast<char *>(buf_[b]) + TSV_FRONT;
    // the other buffer takes the carried line now: this one's tail becomes '\n' padding
    memcpy(static_cast<char *>(buf_[1 - b]) + TSV_FRONT, data + cut_, (size_t)(total_ - cut_));
    memset(data + cut_, '\n', (size_t)TSV_TAIL);
    consumed += cut_;
    ++nchunks;
    return data;
}

void TsvPass::prefetch() {
    fill_rc_ = feed_.fill(static_cast<char *>(buf_[1 - buffer()]) + TSV_FRONT, total_ - cut_, chunk_, cap_, &next_cut_, &next_total_);
    if (fill_rc_ != LDW_OK) fill_err_ = ldw_last_error();   // (the feeder left next_cut_ at 0 or -1: more() is false once the pass advances)
}

void TsvPass::advance() {
    ++k_;
    cut_ = next_cut_;
    total_ = next_total_;
}

int TsvPass::feeder_refusal() const {
    if (fill_rc_ == LDW_OK) return LDW_OK;
    // A line over TSV_LINE_MAX or a read error.  The feeder words the first the same way wherever it meets it (the first chunk, a later one, the last line
    // without its newline), so the saved message alone tells them apart: the cut of -1 it also leaves, in the first chunk or a later one, need not be kept.
    // The line begins where the chunks before it end, at byte `consumed`.
    if (fill_err_.find("longer than") != std::string::npos) {
        int64_t line = 0;
        (void)tsv_line_of_offset(path_, consumed, &line);
        set_error("%s: %s: line %lld, column 1: the line is longer than %lld bytes", who_, path_, (long long)line, (long long)TSV_LINE_MAX);
    } else {
        set_error("%s", fill_err_.c_str());
    }
    return fill_rc_;
}

int TsvPass::refuse_row(int64_t row, uint32_t col, uint32_t reason, int ncols) const {
    int64_t line = 0;
    (void)tsv_line_of_row(path_, row, &line);
    switch (reason) {
    case BAD_MISSING: set_error("%s: %s: line %lld, column %u: the line ends after %u of %d fields", who_, path_, (long long)line, col, col - 1, ncols); break;
    case BAD_EXTRA: set_error("%s: %s: line %lld, column %u: more than %d fields", who_, path_, (long long)line, col, ncols); break;
    case BAD_LONG: set_error("%s: %s: line %lld, column %u: the line is longer than %lld bytes", who_, path_, (long long)line, col, (long long)TSV_LINE_MAX); break;
    default: set_error("%s: %s: line %lld, column %u: not a number", who_, path_, (long long)line, col); break;
    }
    return LDW_ERR_ARG;
}

namespace {
// walks the file line by line: fn(line number (1-based), first byte offset, empty) until it returns true
template <class F>
int walk_lines(const char *path, F fn) {
    errno = 0;
    gzFile f = gzopen(path, "rb");
    LDW_REQUIRE(f != nullptr, LDW_ERR_ARG, "ldw_tsv: cannot open %s: %s", path, errno ? strerror(errno) : "out of memory");
    gzbuffer(f, 1u << 20);
    std::vector<char> buf(1 << 20);
    int64_t line = 1, off = 0, line_off = 0, len = 0;
    char last = 0;
    bool done = false;
    for (int n; !done && (n = gzread(f, buf.data(), (unsigned)buf.size())) > 0;) {
        for (int i = 0; i < n && !done; ++i, ++off) {
            const char ch = buf[(size_t)i];
            if (ch == '\n') {
                const bool empty = len == 0 || (len == 1 && last == '\r');
                done = fn(line, line_off, off, empty);
                ++line;
                line_off = off + 1;
                len = 0;
            } else {
                ++len;
                last = ch;
            }
        }
    }
    if (!done && len > 0) fn(line, line_off, off, len == 1 && last == '\r');
    gzclose(f);
    return LDW_OK;
}
}  // namespace

int tsv_line_of_row(const char *path, int64_t row, int64_t *line_out) {
    int64_t seen = 0;
    *line_out = 0;
    return walk_lines(path, [&](int64_t line, int64_t, int64_t, bool empty) {
        if (empty) return false;
        if (seen++ == row) {
            *line_out = line;
            return true;
        }
        return false;
    });
}

int tsv_line_of_offset(const char *path, int64_t off, int64_t *line_out) {
    *line_out = 0;
    return walk_lines(path, [&](int64_t line, int64_t first, int64_t nl, bool) {
        *line_out = line;
        return off >= first && off <= nl;
    });
}

int tsv_header_columns(const char *path, int64_t line, const char *text, int64_t len, const char *const *names, int n_names, int max_cols, int32_t *col_out,
                       int32_t *ncols_out) {
    if (len > 0 && text[len - 1] == '\r') --len;
    for (int k = 0; k < n_names; ++k) col_out[k] = -1;
    int32_t ncols = 0;
    for (int64_t at = 0; at <= len;) {
        const void *tab = at < len ? memchr(text + at, '\t', (size_t)(len - at)) : nullptr;
        const int64_t end = tab ? (int64_t)(static_cast<const char *>(tab) - text) : len;
        for (int k = 0; k < n_names; ++k)
            if ((int64_t)strlen(names[k]) == end - at && memcmp(names[k], text + at, (size_t)(end - at)) == 0) {
                LDW_REQUIRE(col_out[k] < 0, LDW_ERR_ARG, "ldw_links_grep: %s: line %lld, column %d: the header names \"%s\" twice", path, (long long)line, (int)ncols + 1,
                            names[k]);
                col_out[k] = ncols;
            }
        ++ncols;
        at = end + 1;
    }
    LDW_REQUIRE(ncols <= max_cols, LDW_ERR_ARG, "ldw_links_grep: %s: line %lld, column %d: the header has more than %d columns", path, (long long)line, max_cols + 1,
                max_cols);
    for (int k = 0; k < n_names; ++k)
        LDW_REQUIRE(col_out[k] >= 0, LDW_ERR_ARG, "ldw_links_grep: %s: line %lld, column %d: the header has no column \"%s\"", path, (long long)line, (int)ncols + 1,
                    names[k]);
    *ncols_out = ncols;
    return LDW_OK;
}

double tsv_strtod(const char *p) {
    static locale_t c_locale = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    return strtod_l(p, nullptr, c_locale);
}

}  // namespace ldw

extern "C" {

int ldw_tsv_probe(const char *path, int sep, int32_t *ncols_out, int32_t *gz_out) {
    LDW_REQUIRE(path && ncols_out, LDW_ERR_ARG, "ldw_tsv_probe: null argument");
    LDW_REQUIRE(sep == '\t' || sep == ' ', LDW_ERR_ARG, "ldw_tsv_probe: the separator must be a tab or a space (got %d)", sep);
    errno = 0;
    gzFile f = gzopen(path, "rb");
    LDW_REQUIRE(f != nullptr, LDW_ERR_ARG, "ldw_tsv: cannot open %s: %s", path, errno ? strerror(errno) : "out of memory");
    if (gz_out) *gz_out = gzdirect(f) == 0;
    // the fields of the first non-empty line
    char buf[65536];
    int32_t fields = 0;
    int64_t len = 0;
    char last = 0;
    bool done = false, failed = false;
    for (int n; !done && (n = gzread(f, buf, sizeof(buf))) != 0;) {
        if (n < 0) {
            failed = true;
            break;
        }
        for (int i = 0; i < n && !done; ++i) {
            const char ch = buf[i];
            if (ch == '\n') {
                if (len == 0 || (len == 1 && last == '\r')) {
                    len = 0;
                    fields = 0;
                    continue;
                }
                done = true;
            } else {
                if (len == 0) fields = 1;
                if (ch == (char)sep) ++fields;
                ++len;
                last = ch;
                if (len > ldw::TSV_LINE_MAX) {
                    gzclose(f);
                    ldw::set_error("ldw_tsv_probe: %s: a line is longer than %lld bytes", path, (long long)ldw::TSV_LINE_MAX);
                    return LDW_ERR_ARG;
                }
            }
        }
    }
    gzclose(f);
    LDW_REQUIRE(!failed, LDW_ERR_ARG, "ldw_tsv_probe: reading %s failed", path);
    if (!done && (len == 0 || (len == 1 && last == '\r'))) fields = 0;   // (a last line without a newline counts; a lone '\r' is empty)
    *ncols_out = fields;
    return LDW_OK;
}

}  // extern "C"

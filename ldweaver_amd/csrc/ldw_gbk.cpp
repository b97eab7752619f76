// The native GenBank reader (host only, no context and no GPU): the CDS rows and the reference sequence of a single-record GenBank file
// (plain or gzip), as the reference's parser (R/parseGBK.R, a genbankr fork) gives them to estimate_variation_in_CDS
// (R/estimateCDSDiversity.R:39-47).  The whole file is read with zlib in large chunks and parsed in one pass over its lines; the rules
// and the places they come from are listed in DESIGN.md 17.
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <zlib.h>

#include "ldw_internal.h"

namespace ldw {
namespace {
constexpr unsigned IO_CHUNK = 4u << 20;   // bytes per gzread
const char *const ERR_NOSEQ = "The GBK file should contain the reference sequence!";

inline bool is_space(unsigned char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; }
inline bool is_digit(unsigned char c) { return c >= '0' && c <= '9'; }
inline bool is_upper(unsigned char c) { return c >= 'A' && c <= 'Z'; }
inline bool is_alnum(unsigned char c) { return is_digit(c) || is_upper(c) || (c >= 'a' && c <= 'z'); }
inline bool is_key(unsigned char c) { return is_alnum(c) || c == '\'' || c == '_' || c == '-'; }

struct Line {
    const char *p;
    size_t n;
    bool starts(const char *s, size_t off = 0) const {
        const size_t k = strlen(s);
        return off + k <= n && memcmp(p + off, s, k) == 0;
    }
};

// DNAString's alphabet: IUPAC letters in either case (stored upper case), '-', '+', '.'; 0 = not in it
struct DnaTable {
    unsigned char t[256];
    DnaTable() {
        memset(t, 0, sizeof t);
        for (const char *s = "ACGTMRWSYKVHDBN"; *s; ++s) t[(unsigned char)*s] = t[(unsigned char)(*s + 32)] = (unsigned char)*s;
        t['-'] = '-';
        t['+'] = '+';
        t['.'] = '.';
    }
};
const DnaTable DNA;

std::string shown(const std::string &s) { return s.size() <= 80 ? s : s.substr(0, 77) + "..."; }

struct Feature {
    int64_t line = 0;
    std::string key, loc;
    std::vector<std::string> quals;   // one per qualifier, leading whitespace of each of its lines stripped, the lines joined
};

struct Parsed {
    std::vector<int64_t> start, end, feat;
    std::vector<int8_t> strand;
    std::string seq, meta;
    int64_t nfeat = 0;
};

class Parser {
  public:
    explicit Parser(const char *path) : path_(path) {}
    int run(Parsed &out);

  private:
    const char *path_;
    std::string buf_, origin_, seqname_, locus_, accession_, version_, meta_feat_;
    bool in_feat_ = false, have_feat_ = false, in_origin_ = false, origin_seen_ = false;
    int64_t n_source_rows_ = 0, source_line_ = 0, src_s_ = 0, src_e_ = 0, cds_early_ = 0;
    Feature cur_;
    Parsed *out_ = nullptr;

    int fail(int64_t line, const char *what, const std::string &text) {
        set_error("ldw_gbk: %s: line %lld: %s: '%s'", path_, (long long)line, what, shown(text).c_str());
        return LDW_ERR_ARG;
    }
    int read_file();
    int finish_feature();
    int parse_location(const std::string &s, int64_t line, std::vector<int64_t> &st, std::vector<int64_t> &en, std::vector<int8_t> &sd);
};

int Parser::read_file() {
    errno = 0;
    gzFile f = gzopen(path_, "rb");
    LDW_REQUIRE(f != nullptr, LDW_ERR_ARG, "ldw_gbk: cannot open %s: %s", path_, errno ? strerror(errno) : "out of memory");
    gzbuffer(f, 1u << 20);
    for (;;) {
        const size_t at = buf_.size();
        buf_.resize(at + IO_CHUNK);
        const int n = gzread(f, &buf_[at], IO_CHUNK);
        if (n < 0) {
            int code = 0;
            const char *msg = gzerror(f, &code);
            set_error("ldw_gbk: reading %s failed: %s", path_, msg ? msg : "unknown error");
            gzclose(f);
            return LDW_ERR_ARG;
        }
        buf_.resize(at + (size_t)n);
        if (n == 0) break;
    }
    gzclose(f);
    // '<' and '>' are deleted from the whole text before anything else (parseGenBank, R/parseGBK.R:133)
    if (memchr(buf_.data(), '<', buf_.size()) || memchr(buf_.data(), '>', buf_.size()))
        buf_.erase(std::remove_if(buf_.begin(), buf_.end(), [](char c) { return c == '<' || c == '>'; }), buf_.end());
    return LDW_OK;
}

// loc := complement(inner) | inner ; inner := join(seg, ...) | order(seg, ...) | range ; seg := range | complement(range) ;
// range := a | a..b | a^b (make_feat_gr, .do_join_silliness: R/parseGBK.R:414-489).  Whitespace between tokens is skipped, as as.integer
// skips it in the reference.  A segment with its own complement() inside a join keeps its own strand (the declared divergence).
int Parser::parse_location(const std::string &s, int64_t line, std::vector<int64_t> &st, std::vector<int64_t> &en, std::vector<int8_t> &sd) {
    const char *p = s.data(), *e = p + s.size();
    auto ws = [&] { while (p < e && is_space((unsigned char)*p)) ++p; };
    auto word = [&](const char *w) {
        ws();
        const size_t k = strlen(w);
        if ((size_t)(e - p) >= k && memcmp(p, w, k) == 0) {
            p += k;
            return true;
        }
        return false;
    };
    auto number = [&](int64_t &v) {
        ws();
        if (p == e || !is_digit((unsigned char)*p)) return false;
        v = 0;
        while (p < e && is_digit((unsigned char)*p)) {
            if (v > ((int64_t)1 << 50)) return false;
            v = v * 10 + (*p++ - '0');
        }
        ws();
        return true;
    };
    const char *bad = "a location outside the supported grammar (a, a..b, a^b, complement(), join(), order())";
    auto range = [&](int8_t strand) {
        int64_t a = 0, b = 0;
        if (!number(a)) return fail(line, bad, s);
        if (p + 1 < e && p[0] == '.' && p[1] == '.') {
            p += 2;
            if (!number(b)) return fail(line, bad, s);
        } else if (p < e && *p == '^') {
            ++p;
            if (!number(b)) return fail(line, bad, s);
            b -= 1;
        } else {
            b = a;
        }
        if (b < a - 1) return fail(line, "a segment of negative width (end < start - 1)", s);
        st.push_back(a);
        en.push_back(b);
        sd.push_back(strand);
        return LDW_OK;
    };
    auto seg = [&](int8_t strand, bool in_comp) {
        const char *q = p;
        if (word("complement(")) {
            if (in_comp) return fail(line, "complement() nested in complement()", s);
            if (int rc = range(-1)) return rc;
            if (!word(")")) return fail(line, bad, s);
            return LDW_OK;
        }
        p = q;
        return range(strand);
    };
    auto inner = [&](int8_t strand, bool in_comp) {
        const char *q = p;
        if (word("join(") || (p = q, word("order("))) {
            for (;;) {
                const char *r = p;
                if (word("join(") || (p = r, word("order("))) return fail(line, "join() or order() nested in join() or order()", s);
                p = r;
                if (int rc = seg(strand, in_comp)) return rc;
                if (word(",")) continue;
                if (word(")")) return LDW_OK;
                return fail(line, bad, s);
            }
        }
        p = q;
        return range(strand);
    };
    const char *q = p;
    if (word("complement(")) {
        if (int rc = inner(-1, true)) return rc;
        if (!word(")")) return fail(line, bad, s);
    } else {
        p = q;
        if (int rc = inner(1, false)) return rc;
    }
    ws();
    if (p != e) return fail(line, bad, s);
    return LDW_OK;
}

// the value of qualifier `name` of the current feature: the first one of that name; '/name="v"' -> v, '/name=v' -> v, '/name' -> ""
std::string qualifier(const Feature &f, const char *name) {
    const size_t k = strlen(name);
    for (const std::string &q : f.quals) {
        if (q.size() < k + 1 || q.compare(1, k, name) != 0) continue;
        if (q.size() == k + 1) return std::string();
        if (q[k + 1] != '=') continue;
        size_t a = k + 2, b = q.size();
        if (a < b && q[a] == '"') {
            ++a;
            const size_t c = q.find('"', a);
            if (c != std::string::npos) b = c;
        }
        return q.substr(a, b - a);
    }
    return std::string();
}

bool has_qualifier(const Feature &f, const char *name) {
    const size_t k = strlen(name);
    for (const std::string &q : f.quals)
        if (q.size() >= k + 1 && q.compare(1, k, name) == 0 && (q.size() == k + 1 || q[k + 1] == '=')) return true;
    return false;
}

int Parser::finish_feature() {
    if (!have_feat_) return LDW_OK;
    have_feat_ = false;
    const bool cds = cur_.key == "CDS", source = cur_.key == "source";
    std::vector<int64_t> st, en;
    std::vector<int8_t> sd;
    // every feature's location is checked: the reference builds a GRanges of every feature type
    if (int rc = parse_location(cur_.loc, cur_.line, st, en, sd)) return rc;
    if (source) {
        if (n_source_rows_ == 0) {
            src_s_ = st[0];
            src_e_ = en[0];
            source_line_ = cur_.line;
            // the seqnames of every row: /chromosome, else /strain, else /organism of the source (readFeatures, R/parseGBK.R:560-576)
            const char *which = has_qualifier(cur_, "chromosome") ? "chromosome" : has_qualifier(cur_, "strain") ? "strain" : "organism";
            seqname_ = qualifier(cur_, which);
        }
        n_source_rows_ += (int64_t)st.size();
    } else if (cds) {
        if (n_source_rows_ == 0 && !cds_early_) cds_early_ = cur_.line;
        const int64_t id = out_->nfeat++;
        for (size_t i = 0; i < st.size(); ++i) {
            out_->start.push_back(st[i]);
            out_->end.push_back(en[i]);
            out_->strand.push_back(sd[i]);
            out_->feat.push_back(id);
        }
        for (const char *q : {"locus_tag", "gene", "product"}) meta_feat_.append(qualifier(cur_, q)).push_back('\0');
    }
    return LDW_OK;
}

// ^( {5}|\t)[[:alnum:]'_-]+[[:space:]]+ : *key_end / *loc_at receive the end of the key and the start of what follows the blanks
bool key_line(const Line &l, size_t *key_end, size_t *loc_at) {
    size_t i;
    if (l.starts("     ")) i = 5;
    else if (l.n && l.p[0] == '\t') i = 1;
    else return false;
    const size_t k0 = i;
    while (i < l.n && is_key((unsigned char)l.p[i])) ++i;
    if (i == k0 || i == l.n || !is_space((unsigned char)l.p[i])) return false;
    *key_end = i;
    while (i < l.n && is_space((unsigned char)l.p[i])) ++i;
    *loc_at = i;
    return true;
}

// ^[[:space:]]+/[^[:space:]]+($|=([[:digit:]]|")) (R/parseGBK.R:545)
bool qualifier_line(const Line &l) {
    size_t i = 0;
    while (i < l.n && is_space((unsigned char)l.p[i])) ++i;
    if (i == 0 || i == l.n || l.p[i] != '/') return false;
    const size_t a = ++i;
    while (i < l.n && !is_space((unsigned char)l.p[i])) ++i;
    if (i == a) return false;
    if (i == l.n) return true;
    for (size_t k = a + 1; k + 1 < i; ++k)
        if (l.p[k] == '=' && (is_digit((unsigned char)l.p[k + 1]) || l.p[k + 1] == '"')) return true;
    return false;
}

// ^[[:space:]]*//[[:space:]]*$ : a record break
bool break_line(const Line &l) {
    size_t i = 0;
    while (i < l.n && is_space((unsigned char)l.p[i])) ++i;
    if (!(i + 1 < l.n && l.p[i] == '/' && l.p[i + 1] == '/')) return false;
    for (i += 2; i < l.n; ++i)
        if (!is_space((unsigned char)l.p[i])) return false;
    return true;
}

void strip_lead(const Line &l, std::string &to) {
    size_t i = 0;
    while (i < l.n && is_space((unsigned char)l.p[i])) ++i;
    to.append(l.p + i, l.n - i);
}

// the first whitespace-delimited token after the field name
std::string field_token(const Line &l) {
    size_t i = 0;
    while (i < l.n && is_upper((unsigned char)l.p[i])) ++i;
    while (i < l.n && is_space((unsigned char)l.p[i])) ++i;
    size_t j = i;
    while (j < l.n && !is_space((unsigned char)l.p[j])) ++j;
    return std::string(l.p + i, j - i);
}

int Parser::run(Parsed &out) {
    out_ = &out;
    if (int rc = read_file()) return rc;
    const char *b = buf_.data();
    const size_t n = buf_.size();
    // records: LOCUS lines and '//' lines (readGenBank2's multi-record branch, R/parseGBK.R:105-112, cannot produce a record)
    int64_t n_locus = 0, n_break = 0;
    for (size_t p = 0, lineno = 1; p < n; ++lineno) {
        size_t q = p;
        while (q < n && b[q] != '\n' && b[q] != '\r') ++q;
        const Line l{b + p, q - p};
        p = q < n ? (b[q] == '\r' && q + 1 < n && b[q + 1] == '\n' ? q + 2 : q + 1) : n;
        if (l.n && is_upper((unsigned char)l.p[0])) {   // a field starts (R/parseGBK.R:130, :143-147)
            if (in_feat_) {
                if (int rc = finish_feature()) return rc;
            }
            size_t k = 0;
            while (k < l.n && is_upper((unsigned char)l.p[k])) ++k;
            const std::string name(l.p, k);
            in_feat_ = name == "FEATURES";
            in_origin_ = name == "ORIGIN";
            origin_seen_ |= in_origin_;
            if (name == "LOCUS") {
                if (n_locus++ == 0) locus_ = field_token(l);
            } else if (name == "ACCESSION" && accession_.empty()) {
                accession_ = field_token(l);
            } else if (name == "VERSION" && version_.empty()) {
                version_ = field_token(l);
            }
            continue;
        }
        if (break_line(l)) ++n_break;
        if (in_origin_) {   // readOrigin (R/parseGBK.R:599-612): whitespace, digits and '//' go; DNAString's alphabet, upper case
            for (size_t i = 0; i < l.n; ++i) {
                const unsigned char c = (unsigned char)l.p[i];
                if (is_space(c) || is_digit(c)) continue;
                if (c == '/' && i + 1 < l.n && l.p[i + 1] == '/') {
                    ++i;
                    continue;
                }
                const unsigned char u = DNA.t[c];
                if (!u) {
                    char what[96];
                    snprintf(what, sizeof what, "character '%c' (%u) of the ORIGIN sequence is not an IUPAC DNA letter or one of -+.", c >= 32 && c < 127 ? c : '?', c);
                    return fail((int64_t)lineno, what, std::string(l.p, l.n));
                }
                origin_.push_back((char)u);
            }
        } else if (in_feat_) {
            size_t key_end = 0, loc_at = 0;
            if (key_line(l, &key_end, &loc_at)) {
                const unsigned char c = loc_at < l.n ? (unsigned char)l.p[loc_at] : 0;
                const bool feature = is_digit(c) || c == ',' || l.starts("complement", loc_at) || l.starts("join", loc_at) || l.starts("order", loc_at);
                if (feature) {   // a feature starts (R/parseGBK.R:519)
                    if (int rc = finish_feature()) return rc;
                    size_t k0 = 0;
                    while (is_space((unsigned char)l.p[k0])) ++k0;
                    cur_.line = (int64_t)lineno;
                    cur_.key.assign(l.p + k0, key_end - k0);
                    cur_.loc.assign(l.p + loc_at, l.n - loc_at);
                    cur_.quals.clear();
                    have_feat_ = true;
                    continue;
                }
                if (c) return fail((int64_t)lineno, "a feature location outside the supported grammar (a remote accession, gap(), one-of(), ...)",
                                   std::string(l.p, l.n));
            }
            if (!have_feat_) continue;   // lines between FEATURES and the first feature
            if (qualifier_line(l)) {
                cur_.quals.emplace_back();
                strip_lead(l, cur_.quals.back());
            } else {
                strip_lead(l, cur_.quals.empty() ? cur_.loc : cur_.quals.back());
            }
        }
    }
    if (in_feat_) {
        if (int rc = finish_feature()) return rc;
    }
    const int64_t records = std::max(n_locus, n_break);
    LDW_REQUIRE(records <= 1, LDW_ERR_ARG, "ldw_gbk: %s holds %lld GenBank records (%lld LOCUS lines, %lld '//' lines): only a single-record file is "
                "supported", path_, (long long)records, (long long)n_locus, (long long)n_break);
    LDW_REQUIRE(n_locus == 1, LDW_ERR_ARG, "ldw_gbk: %s has no LOCUS line: not a GenBank file", path_);
    LDW_REQUIRE(origin_seen_ && !origin_.empty(), LDW_ERR_ARG, "%s (ldw_gbk: %s has no ORIGIN sequence)", ERR_NOSEQ, path_);
    LDW_REQUIRE(n_source_rows_ == 1, LDW_ERR_ARG, "%s (ldw_gbk: %s has %lld source ranges, the reference cuts its sequence to exactly one)", ERR_NOSEQ,
                path_, (long long)n_source_rows_);
    LDW_REQUIRE(!cds_early_, LDW_ERR_ARG, "ldw_gbk: %s: line %lld: a CDS feature before the source feature (its rows would have no sequence "
                "name; the reference fails on them)", path_, (long long)cds_early_);
    // the sequence is cut to the source's range (extractAt, R/parseGBK.R:175-185)
    LDW_REQUIRE(src_s_ >= 1 && src_e_ <= (int64_t)origin_.size(), LDW_ERR_ARG, "ldw_gbk: %s: line %lld: the source feature spans %lld..%lld, outside the "
                "ORIGIN sequence of %zu characters", path_, (long long)source_line_, (long long)src_s_, (long long)src_e_, origin_.size());
    out.seq.assign(origin_, (size_t)(src_s_ - 1), (size_t)(src_e_ - src_s_ + 1));
    for (const std::string *s : {&seqname_, &locus_, &accession_, &version_}) out.meta.append(*s).push_back('\0');
    out.meta.append(meta_feat_);
    return LDW_OK;
}

}  // namespace
}  // namespace ldw

using namespace ldw;

extern "C" {

int ldw_gbk_probe(const char *path, int64_t *n_rows, int64_t *n_features, int64_t *g, int64_t *meta_bytes) {
    LDW_REQUIRE(path && n_rows && n_features && g && meta_bytes, LDW_ERR_ARG, "ldw_gbk_probe: null argument");
    Parsed r;
    if (int rc = Parser(path).run(r)) return rc;
    *n_rows = (int64_t)r.start.size();
    *n_features = r.nfeat;
    *g = (int64_t)r.seq.size();
    *meta_bytes = (int64_t)r.meta.size();
    return LDW_OK;
}

int ldw_gbk_read(const char *path, int64_t rows_cap, int64_t *start, int64_t *end, int8_t *strand, int64_t *feature, int64_t g_cap, char *seq,
                 int64_t meta_cap, char *meta) {
    LDW_REQUIRE(path && start && end && strand && feature && seq && meta, LDW_ERR_ARG, "ldw_gbk_read: null argument");
    Parsed r;
    if (int rc = Parser(path).run(r)) return rc;
    const int64_t nr = (int64_t)r.start.size(), g = (int64_t)r.seq.size(), nm = (int64_t)r.meta.size();
    LDW_REQUIRE(rows_cap >= nr && g_cap >= g && meta_cap >= nm, LDW_ERR_SIZE, "ldw_gbk_read: %s needs %lld rows, %lld sequence bytes and %lld metadata "
                "bytes; the buffers hold %lld, %lld and %lld", path, (long long)nr, (long long)g, (long long)nm, (long long)rows_cap,
                (long long)g_cap, (long long)meta_cap);
    memcpy(start, r.start.data(), (size_t)nr * sizeof(int64_t));
    memcpy(end, r.end.data(), (size_t)nr * sizeof(int64_t));
    memcpy(strand, r.strand.data(), (size_t)nr);
    memcpy(feature, r.feat.data(), (size_t)nr * sizeof(int64_t));
    memcpy(seq, r.seq.data(), (size_t)g);
    memcpy(meta, r.meta.data(), (size_t)nm);
    return LDW_OK;
}

}  // extern "C"

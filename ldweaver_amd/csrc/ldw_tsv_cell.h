// One numeric cell of a text table on the device (include/ldweaver_amd.h 13): the grammar and the value rule that the reader of numeric
// link tables (ldw_links_read.hip) and the search of annotated link files (ldw_links_grep.hip) share.
// No contraction in a file that includes this: m * 1e^k must be rounded once, as a product.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ldw {

enum { CELL_OK = 0, CELL_SLOW = 1, CELL_BAD = 2 };

static __device__ const double kPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                             1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

__device__ __forceinline__ bool is_digit(uint8_t c) { return (uint8_t)(c - '0') <= 9; }

// The cell that starts at p[i]: i moves to the first byte the number does not take (the caller checks that it is a separator or the end of the line).
// CELL_OK: v is its value (Clinger's fast path, NA / NaN / Inf tokens).  CELL_SLOW: a number whose value the host's strtod must give (v = 0).
// CELL_BAD: not a number (i is then undefined).  plain: the cell is an integer literal [+-]?[0-9]+.  Reads at most three bytes past a byte that is
// neither a separator nor a line end.
template <class P>
__device__ __forceinline__ int parse_cell(P p, uint32_t &i, double &v, bool &plain) {
    uint8_t c = p[i];
    bool neg = false, sgn = false;
    if (c == '-' || c == '+') {
        neg = c == '-';
        sgn = true;
        c = p[++i];
    }
    plain = true;
    if (is_digit(c) || c == '.') {
        uint64_t m = 0;
        int nd = 0, dexp = 0;
        bool any = false, dropped = false;
        while (is_digit(c)) {
            any = true;
            const uint32_t d = c - '0';
            if (m != 0 || d != 0) {
                if (nd < 19) {
                    m = m * 10 + d;
                    ++nd;
                } else {
                    dropped = true;
                    if (dexp < 100000) ++dexp;
                }
            }
            c = p[++i];
        }
        if (c == '.') {
            plain = false;
            c = p[++i];
            while (is_digit(c)) {
                any = true;
                const uint32_t d = c - '0';
                if (m != 0 || d != 0) {
                    if (nd < 19) {
                        m = m * 10 + d;
                        ++nd;
                        --dexp;
                    } else {
                        dropped = true;
                    }
                } else if (dexp > -100000) {
                    --dexp;
                }
                c = p[++i];
            }
        }
        if (!any) return CELL_BAD;
        if (c == 'e' || c == 'E') {
            plain = false;
            c = p[++i];
            bool eneg = false;
            if (c == '-' || c == '+') {
                eneg = c == '-';
                c = p[++i];
            }
            if (!is_digit(c)) return CELL_BAD;
            int e = 0;
            while (is_digit(c)) {
                if (e < 100000) e = e * 10 + (c - '0');
                c = p[++i];
            }
            dexp += eneg ? -e : e;
        }
        if (m == 0) {
            v = 0.0;
        } else if (!dropped && m <= (1ull << 53) && dexp >= -22 && dexp <= 22) {
            const double dm = (double)m;   // exact
            v = dexp < 0 ? dm / kPow10[-dexp] : dm * kPow10[dexp];
        } else {
            v = 0.0;
            return CELL_SLOW;
        }
        if (neg) v = -v;
        return CELL_OK;
    }
    plain = false;
    if (!sgn && c == 'N' && p[i + 1] == 'A') {
        v = __longlong_as_double(0x7ff8000000000000ll);
        i += 2;
    } else if (!sgn && ((c == 'N' && p[i + 1] == 'a' && p[i + 2] == 'N') || (c == 'n' && p[i + 1] == 'a' && p[i + 2] == 'n'))) {
        v = __longlong_as_double(0x7ff8000000000000ll);
        i += 3;
    } else if ((!sgn || neg) && (c == 'I' || c == 'i') && p[i + 1] == 'n' && p[i + 2] == 'f') {
        v = __longlong_as_double(neg ? 0xfff0000000000000ll : 0x7ff0000000000000ll);
        i += 3;
    } else {
        return CELL_BAD;
    }
    return CELL_OK;
}

}  // namespace ldw

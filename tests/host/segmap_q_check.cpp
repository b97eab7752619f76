// The fixed-point rule of the segment map (ldweaver_amd/csrc/ldw_segmap.h) on the HOST: reads doubles as 16 hex digits of their bits, one per line, from
// standard input and prints "q lo hi refused snpsum_q" for each; tests/test_segmap_host.py compares the lines with numpy's rint and with the per-SNP
// summary's rule.  Plain C++: g++ only.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../ldweaver_amd/csrc/ldw_segmap.h"

int main() {
    static_assert(ldw::SNPSUM_FRAC == 40 && ldw::SEGMAP_LO_BITS == 24, "q = llrint(v 2^40), split at bit 24");
    char line[64];
    long n = 0;
    while (fgets(line, sizeof line, stdin)) {
        uint64_t u = 0;
        if (sscanf(line, "%" SCNx64, &u) != 1) continue;
        double v;
        memcpy(&v, &u, 8);
        bool refused = false, refused21 = false;
        const int64_t q = ldw::segmap_q(v, &refused);
        int64_t lo = 0, hi = 0;
        ldw::segmap_split(q, &lo, &hi);
        const int64_t q21 = ldw::snpsum_q(v, &refused21);
        printf("%" PRId64 " %" PRId64 " %" PRId64 " %d %" PRId64 "\n", q, lo, hi, refused ? 1 : 0, q21);
        ++n;
    }
    fprintf(stderr, "values %ld\n", n);
    return 0;
}

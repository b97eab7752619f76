// The fixed-point rule of the per-SNP MI summary (ldweaver_amd/csrc/ldw_snpsum.h) on the HOST: reads doubles as 16 hex digits of their bits, one per line,
// from standard input and prints "q refused" for each; tests/test_background_host.py compares the lines with numpy's rint.  Plain C++: g++ only.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../ldweaver_amd/csrc/ldw_snpsum.h"

int main() {
    static_assert(ldw::SNPSUM_FRAC == 40, "the scale of snpsum_q is 2^40");
    char line[64];
    long n = 0;
    while (fgets(line, sizeof line, stdin)) {
        uint64_t u = 0;
        if (sscanf(line, "%" SCNx64, &u) != 1) continue;
        double v;
        memcpy(&v, &u, 8);
        bool refused = false;
        const int64_t q = ldw::snpsum_q(v, &refused);
        printf("%" PRId64 " %d\n", q, refused ? 1 : 0);
        ++n;
    }
    fprintf(stderr, "values %ld\n", n);
    return 0;
}

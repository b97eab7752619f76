// The corrected score of a SNP pair (ldweaver_amd/csrc/ldw_score.h) on the HOST: reads three doubles per line (mi, wa, wb) as 16 hex digits of their bits
// from standard input and prints the bits of the score; tests/test_apc_links_host.py compares the lines with numpy's product and difference.  Plain C++:
// g++ only.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../ldweaver_amd/csrc/ldw_score.h"

int main() {
    char line[128];
    long n = 0;
    while (fgets(line, sizeof line, stdin)) {
        uint64_t u[3] = {0, 0, 0};
        if (sscanf(line, "%" SCNx64 " %" SCNx64 " %" SCNx64, &u[0], &u[1], &u[2]) != 3) continue;
        double v[3];
        memcpy(v, u, sizeof v);
        const double s = ldw::pair_score(v[0], v[1], v[2]);
        uint64_t out;
        memcpy(&out, &s, 8);
        printf("%016" PRIx64 "\n", out);
        ++n;
    }
    fprintf(stderr, "values %ld\n", n);
    return 0;
}

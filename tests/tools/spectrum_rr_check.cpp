// spectrum_rr_check.cpp -- score_spectrum_rr.hpp on pencils from a file, stand-alone (tests/test_spectrum_host.py builds it
// with the host sanitizers and runs it as a child process; it is never loaded into Python and needs no GPU).
//
//   spectrum_rr_check IN OUT [indefinite]
// A third argument, whatever it says, selects the indefinite rule (score_curvature.hpp): the lowest value may be negative.
// IN : count, then per pencil "m nb" and the 2 m m entries of S'AS and S'S (row-major, %.17g).
// OUT: per pencil "status kept", nb Ritz values, m nb coefficients (row-major).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "score_spectrum_rr.hpp"

int main(int argc, char** argv) {
    if (argc != 3 && argc != 4) { std::fprintf(stderr, "usage: %s IN OUT [indefinite]\n", argv[0]); return 2; }
    const bool indefinite = argc == 4;
    std::FILE* in = std::fopen(argv[1], "r");
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::FILE* out = std::fopen(argv[2], "w");
    if (!out) { std::fprintf(stderr, "cannot write %s\n", argv[2]); std::fclose(in); return 2; }
    int count = 0, rc = 0;
    if (std::fscanf(in, "%d", &count) != 1 || count < 0) rc = 3;
    for (int p = 0; p < count && rc == 0; ++p) {
        int m = 0, nb = 0;
        if (std::fscanf(in, "%d %d", &m, &nb) != 2 || m < 1 || m > 4096 || nb < 1 || m != 3 * nb) { rc = 3; break; }
        const size_t mm = (size_t)m * (size_t)m;
        std::vector<double> GA(mm), GB(mm), theta((size_t)nb), C((size_t)m * (size_t)nb);
        for (size_t i = 0; i < mm && rc == 0; ++i)
            if (std::fscanf(in, "%lf", &GA[i]) != 1) rc = 3;
        for (size_t i = 0; i < mm && rc == 0; ++i)
            if (std::fscanf(in, "%lf", &GB[i]) != 1) rc = 3;
        if (rc) break;
        int kept = 0;
        const int status = score::sp_rayleigh_ritz(m, nb, GA.data(), GB.data(), theta.data(), C.data(), &kept, indefinite);
        std::fprintf(out, "%d %d\n", status, kept);
        for (double v : theta) std::fprintf(out, "%.17g\n", v);
        for (double v : C) std::fprintf(out, "%.17g\n", v);
    }
    std::fclose(in);
    if (std::fclose(out) != 0) rc = 4;
    if (rc) std::fprintf(stderr, "spectrum_rr_check: bad input (%d)\n", rc);
    return rc;
}

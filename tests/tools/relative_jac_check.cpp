// relative_jac_check.cpp -- rp_pair_jac of csrc/score_relative.hpp on the host, stand-alone (tests/test_relative_host.py builds
// it with g++, plain and under the host sanitizers): the text the device kernels compile, at points read from a file.
//
// Input (argv[1]), numbers as C99 hexadecimal floats:  dim Np C, then the state of the Np poses in the library's layout
// (2-D [theta, x, y], 3-D [R row-major | t] per pose), then C pairs "a b".
// Output, one line per pair: "pair a b", then R_ab (dim x dim), t_ab (dim) and G (dp x 2 dp, row-major) as hexadecimal floats.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "score_relative.hpp"

template <int DIM>
static int run(const std::vector<double>& X, long long Np, const std::vector<long long>& pairs) {
    constexpr int DP = DIM == 2 ? 3 : 6;
    score::GnView v{};
    v.Np = Np; v.Nl = 0; v.X = X.data();
    for (size_t c = 0; c + 1 < pairs.size(); c += 2) {
        double R[DIM * DIM], t[DIM], G[DP * 2 * DP];
        score::rp_pair_jac<DIM>(v, pairs[c], pairs[c + 1], R, t, G);
        std::printf("pair %lld %lld", pairs[c], pairs[c + 1]);
        for (double x : R) std::printf(" %a", x);
        for (double x : t) std::printf(" %a", x);
        for (double x : G) std::printf(" %a", x);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: relative_jac_check FILE\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    long long dim = 0, Np = 0, C = 0;
    if (std::fscanf(f, "%lld %lld %lld", &dim, &Np, &C) != 3 || (dim != 2 && dim != 3) || Np < 1 || C < 0) {
        std::fprintf(stderr, "bad header\n");
        std::fclose(f);
        return 2;
    }
    std::vector<double> X((size_t)(Np * (dim == 2 ? 3 : 12)));
    char word[64];
    for (double& x : X) {
        if (std::fscanf(f, "%63s", word) != 1) { std::fprintf(stderr, "short state\n"); std::fclose(f); return 2; }
        x = std::strtod(word, nullptr);
    }
    std::vector<long long> pairs((size_t)(2 * C));
    for (long long& p : pairs) {
        if (std::fscanf(f, "%lld", &p) != 1 || p < 0 || p >= Np) { std::fprintf(stderr, "bad pair\n"); std::fclose(f); return 2; }
    }
    std::fclose(f);
    return dim == 2 ? run<2>(X, Np, pairs) : run<3>(X, Np, pairs);
}

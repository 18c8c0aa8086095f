// curvature_blocks_check.cpp -- the exact blocks of score_gn.hpp (J'J plus the curvature term sum_q r_q grad^2 r_q) against
// Richardson-extrapolated central differences of the EXISTING gradient J'r, stand-alone (tests/test_curvature_host.py builds
// it with g++, plain and with the host sanitizers, and runs it as a child process; it is never loaded into Python and needs
// no GPU).
//
//   curvature_blocks_check [BOUND]
// For each of the four block kinds with a curvature term -- relative pose 2-D and 3-D, range 2-D and 3-D -- at 64 seeded
// points with residuals of order 1 after whitening: column b of the reference is d (J'r) / d x_b,
//   D(h) = (g(x + h e_b) - g(x - h e_b)) / (2 h),   (4 D(h / 2) - D(h)) / 3,   h = 2^-9,
// whose truncation error is O(h^4) and whose rounding error is eps |g| / h.  In 3-D a pose moves by the retraction
// R Exp(omega), and the gradient at the moved point is in THAT point's tangent coordinates, which differ from the
// retraction's by -(omega x g) / 2 + O(omega^2): its derivative is antisymmetric, E is symmetric, so the symmetric part of the
// difference matrix is compared (in 2-D it is symmetric by itself, to the differences' error).
// Before comparing, the curvature part (exact block - J'J block) must be at least 1e-2 of the block's largest entry: a
// formula error is of order 1 relative to that part.  Prints one line per kind, "kind worst_discrepancy least_share", the
// discrepancy relative to the block's largest entry; returns 1 where a share is below 1e-2 or a discrepancy above BOUND
// (default: not tested).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "score_gn.hpp"

namespace {

struct Rng {  // splitmix64: the points are the same everywhere
    uint64_t s;
    double uniform() {  // (-1, 1)
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        return (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
    }
};

struct Worst { double discrepancy = 0.0, share = INFINITY; };

// N local unknowns; block(x, H, g, exact) evaluates at the point moved by the local step x
template <int N, class Block>
void compare(Block block, Worst& w) {
    const double h = 1.0 / 512.0;
    double E[N * N], H[N * N], g[N], x[N] = {};
    block(x, E, g, true);
    block(x, H, g, false);
    double D[N * N];
    for (int b = 0; b < N; ++b) {
        double d1[N], d2[N], gp[N], gm[N], scratch[N * N];
        for (int pass = 0; pass < 2; ++pass) {
            const double hh = pass ? 0.5 * h : h;
            x[b] = hh; block(x, scratch, gp, false);
            x[b] = -hh; block(x, scratch, gm, false);
            x[b] = 0.0;
            for (int a = 0; a < N; ++a) (pass ? d2 : d1)[a] = (gp[a] - gm[a]) / (2.0 * hh);
        }
        for (int a = 0; a < N; ++a) D[a * N + b] = (4.0 * d2[a] - d1[a]) / 3.0;
    }
    double top = 0.0, part = 0.0, worst = 0.0;
    for (int k = 0; k < N * N; ++k) { top = std::fmax(top, std::fabs(E[k])); part = std::fmax(part, std::fabs(E[k] - H[k])); }
    for (int a = 0; a < N; ++a)
        for (int b = 0; b < N; ++b) worst = std::fmax(worst, std::fabs(E[a * N + b] - 0.5 * (D[a * N + b] + D[b * N + a])));
    w.discrepancy = std::fmax(w.discrepancy, worst / top);
    w.share = std::fmin(w.share, part / top);
}

void random_rotation(Rng& r, double* R) {
    const double w[3] = {2.0 * r.uniform(), 2.0 * r.uniform(), 2.0 * r.uniform()};
    score::gn_so3_exp(w, R);
}

}  // namespace

int main(int argc, char** argv) {
    const double bound = argc > 1 ? std::atof(argv[1]) : INFINITY;
    const int points = 64;
    Worst rel2, rng2, rel3, rng3;
    Rng r{20240611ull};
    for (int p = 0; p < points; ++p) {
        {   // relative pose, 2-D: residuals of order 1 from offsets of order 1 under precisions of order 1
            const double pi[3] = {3.0 * r.uniform(), 2.0 * r.uniform(), 2.0 * r.uniform()};
            const double pj[3] = {3.0 * r.uniform(), 2.0 * r.uniform(), 2.0 * r.uniform()};
            const double tm[2] = {1.0 + r.uniform(), r.uniform()};
            const double th = 3.0 * r.uniform();
            const double Rm[4] = {std::cos(th), -std::sin(th), std::sin(th), std::cos(th)};
            const double kappa = 2.0 + r.uniform(), tau = 2.0 + r.uniform();
            compare<6>([&](const double* x, double* H, double* g, bool exact) {
                score::gn_rel_block(pi[0] + x[0], pi[1] + x[1], pi[2] + x[2], pj[0] + x[3], pj[1] + x[4], pj[2] + x[5], tm, Rm, kappa, tau, H,
                                    g, exact);
            }, rel2);
        }
        {   // range, 2-D: the points 1..4 apart, the measured distance off by order 1
            const double a[2] = {2.0 * r.uniform(), 2.0 * r.uniform()};
            const double ang = 3.0 * r.uniform(), sep = 2.5 + 1.5 * r.uniform();
            const double b[2] = {a[0] + sep * std::cos(ang), a[1] + sep * std::sin(ang)};
            const double off = r.uniform(), dist = sep + (off < 0 ? off - 0.5 : off + 0.5), prec = 1.5 + r.uniform();
            compare<4>([&](const double* x, double* H, double* g, bool exact) {
                score::gn_range_block(a[0] + x[0], a[1] + x[1], b[0] + x[2], b[1] + x[3], dist, prec, H, g, exact);
            }, rng2);
        }
        {   // relative pose, 3-D: the poses move by the retraction
            double Xi[12], Xj[12], Rm[9];
            random_rotation(r, Xi); random_rotation(r, Xj); random_rotation(r, Rm);
            for (int k = 0; k < 3; ++k) { Xi[9 + k] = 2.0 * r.uniform(); Xj[9 + k] = 2.0 * r.uniform(); }
            const double tm[3] = {1.0 + r.uniform(), r.uniform(), r.uniform()};
            const double kappa = 2.0 + r.uniform(), tau = 2.0 + r.uniform();
            compare<12>([&](const double* x, double* H, double* g, bool exact) {
                double Yi[12], Yj[12];
                score::gn_pose3_retract(Xi, x, Yi);
                score::gn_pose3_retract(Xj, x + 6, Yj);
                score::gn_rel_block3(Yi, Yj, tm, Rm, kappa, tau, H, g, exact);
            }, rel3);
        }
        {   // range, 3-D
            const double a[3] = {2.0 * r.uniform(), 2.0 * r.uniform(), 2.0 * r.uniform()};
            double dir[3] = {r.uniform(), r.uniform(), r.uniform() + 1.5};
            const double nrm = std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]), sep = 2.5 + 1.5 * r.uniform();
            const double b[3] = {a[0] + sep * dir[0] / nrm, a[1] + sep * dir[1] / nrm, a[2] + sep * dir[2] / nrm};
            const double off = r.uniform(), dist = sep + (off < 0 ? off - 0.5 : off + 0.5), prec = 1.5 + r.uniform();
            compare<6>([&](const double* x, double* H, double* g, bool exact) {
                const double pa[3] = {a[0] + x[0], a[1] + x[1], a[2] + x[2]}, pb[3] = {b[0] + x[3], b[1] + x[4], b[2] + x[5]};
                score::gn_range_block3(pa, pb, dist, prec, H, g, exact);
            }, rng3);
        }
    }
    const char* names[4] = {"rel2", "range2", "rel3", "range3"};
    const Worst* all[4] = {&rel2, &rng2, &rel3, &rng3};
    int rc = 0;
    for (int k = 0; k < 4; ++k) {
        std::printf("%s %.6e %.6e\n", names[k], all[k]->discrepancy, all[k]->share);
        if (!(all[k]->share >= 1e-2)) { std::fprintf(stderr, "%s: the curvature part is only %.3e of the block\n", names[k], all[k]->share); rc = 1; }
        if (!(all[k]->discrepancy <= bound)) { std::fprintf(stderr, "%s: discrepancy %.3e above %.3e\n", names[k], all[k]->discrepancy, bound); rc = 1; }
    }
    return rc;
}

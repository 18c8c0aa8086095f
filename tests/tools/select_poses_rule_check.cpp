// select_poses_rule_check.cpp -- the rule of the greedy selection of loop closures (score_select_poses_rule.hpp: selp_gain,
// selp_stop, selp_scaled, selp_weights, selp_check, selp_greedy_host) on tables written by hand: no device, no library.  Each
// table is a matrix P (N x N, N = C DP) with the candidates' precisions, the exclusions, k and min_gain; A = I + D (P + P')/2 D
// is formed here the way k_sel_sym forms it.  Where the answer can be worked out on paper (blocks that are multiples of the
// identity) it is stated with the table; on the coupled tables the sum of the gains is held to 1/2 logdet A_SS from an
// unpivoted Cholesky factorisation of the picked rows and columns written here.  Between them the tables must reach every exit
// of the rule -- all k picked, nothing eligible, no gain, the min_gain stop -- a tie, a duplicate, an excluded candidate and
// every argument error; the program exits non-zero if one was not.  Every table is printed with what the routine returned
// (%.17g), so that the NumPy restatement can be held to the same numbers; the last line is "every branch reached".
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I score_amd/csrc select_poses_rule_check.cpp
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "score_select_poses_rule.hpp"

using namespace score;

namespace {

int failures = 0;
void fail(const std::string& where, const std::string& what) {
    std::fprintf(stderr, "FAIL %s: %s\n", where.c_str(), what.c_str());
    ++failures;
}
bool close(double a, double b, double ulps = 4.0) { return std::fabs(a - b) <= ulps * 1.2e-16 * std::fmax(1.0, std::fabs(b)); }

enum Exit { kAll = 0, kNoneEligible, kNoGain, kMinGain, kExits };
bool reached[kExits] = {false, false, false, false};
bool saw_tie = false, saw_excluded = false, saw_duplicate = false;

struct Table {
    std::string name;
    int dim;
    int32_t C, k;
    double min_gain;
    std::vector<double> P, kappa, tau;
    std::vector<int32_t> excluded;   // empty: none
    int32_t picked;
    std::vector<int32_t> order;      // k
};
struct Result {
    std::vector<int32_t> order;
    std::vector<double> gains, pick, remaining, A, w;
};

// A = I + D (P + P')/2 D, an entry formed once per unordered pair of indices (k_sel_sym's order)
std::vector<double> form_A(const std::vector<double>& P, const std::vector<double>& w) {
    const size_t N = w.size();
    std::vector<double> A(N * N);
    for (size_t r = 0; r < N; ++r)
        for (size_t c = 0; c < N; ++c) {
            const size_t lo = r < c ? r : c, hi = r < c ? c : r;
            const double s = 0.5 * (P[r * N + c] + P[c * N + r]);
            const double v = (std::sqrt(w[lo]) * s) * std::sqrt(w[hi]);
            A[r * N + c] = r == c ? 1.0 + v : v;
        }
    return A;
}

// 1/2 logdet of the rows and columns `idx` of A (N x N) by an unpivoted Cholesky factorisation; NAN where it breaks down
double half_logdet(const std::vector<double>& A, size_t N, const std::vector<size_t>& idx) {
    const size_t n = idx.size();
    std::vector<double> M(n * n);
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < n; ++j) M[i * n + j] = A[idx[i] * N + idx[j]];
    double s = 0.0;
    for (size_t q = 0; q < n; ++q) {
        double pi = M[q * n + q];
        for (size_t m = 0; m < q; ++m) pi -= M[q * n + m] * M[q * n + m];
        if (!(pi > 0.0)) return NAN;
        s += std::log(pi);
        const double root = std::sqrt(pi);
        for (size_t i = q + 1; i < n; ++i) {
            double acc = M[i * n + q];
            for (size_t m = 0; m < q; ++m) acc -= M[i * n + m] * M[q * n + m];
            M[i * n + q] = acc / root;
        }
    }
    return 0.5 * s;
}

template <class T>
void print_row(const char* label, const std::vector<T>& v) {
    std::printf("%s", label);
    for (const T& x : v) std::printf(" %.17g", (double)x);
    std::printf("\n");
}

template <int DP>
Result run_dp(const Table& t) {
    const size_t C = (size_t)t.C, k = (size_t)t.k, N = C * DP, BB = DP * DP;
    Result R;
    R.w.resize(N);
    selp_weights(t.C, t.dim, t.kappa.data(), t.tau.data(), R.w.data());
    R.A = form_A(t.P, R.w);
    R.order.assign(k, -9);
    R.gains.assign(k, -9.0); R.pick.assign(k * BB, -9.0); R.remaining.assign(C * BB, -9.0);
    std::vector<int32_t> state(C);
    std::vector<double> B(C * BB), L(N * k * DP, 0.0);
    const int32_t got = selp_greedy_host<DP>(R.A.data(), R.w.data(), t.excluded.empty() ? nullptr : t.excluded.data(), t.C, t.k, t.min_gain,
                                             R.order.data(), R.gains.data(), R.pick.data(), R.remaining.data(), B.data(), state.data(),
                                             L.data());
    if (got != t.picked) fail(t.name, "picked " + std::to_string(got) + ", expected " + std::to_string(t.picked));
    if (R.order != t.order) fail(t.name, "the order differs");
    // the gains add up to 1/2 logdet of the picked rows and columns and do not increase, and no eligible candidate would have
    // added more than the pick did (by 1/2 logdet of the enlarged set, not by the routine's own blocks)
    std::vector<size_t> idx;
    double total = 0.0;
    for (int32_t j = 0; j < got; ++j) {
        const double before = j ? half_logdet(R.A, N, idx) : 0.0;
        for (size_t c = 0; c < C; ++c) {
            bool taken = !t.excluded.empty() && t.excluded[c];
            for (int32_t i = 0; i < j; ++i) taken = taken || R.order[(size_t)i] == (int32_t)c;
            if (taken) continue;
            std::vector<size_t> with = idx;
            for (int q = 0; q < DP; ++q) with.push_back(c * DP + q);
            if (half_logdet(R.A, N, with) - before > R.gains[(size_t)j] * (1.0 + 1e-12) + 1e-12)
                fail(t.name, "candidate " + std::to_string(c) + " would have added more than pick " + std::to_string(j));
        }
        for (int q = 0; q < DP; ++q) idx.push_back((size_t)R.order[(size_t)j] * DP + q);
        total += R.gains[(size_t)j];
        if (!close(total, half_logdet(R.A, N, idx), 64.0)) fail(t.name, "the gains of the first " + std::to_string(j + 1) + " picks against 1/2 logdet");
        if (j > 0 && !(R.gains[(size_t)j] <= R.gains[(size_t)j - 1] * (1.0 + 1e-15))) fail(t.name, "the gains increase");
        for (size_t e = 0; e < BB; ++e)
            if (R.remaining[(size_t)R.order[(size_t)j] * BB + e] != R.pick[(size_t)j * BB + e]) fail(t.name, "a picked candidate keeps the value at its pick");
    }
    for (size_t j = (size_t)got; j < k; ++j) {
        if (R.order[j] != -1 || R.gains[j] != 0.0) fail(t.name, "the padding of order and gains");
        for (size_t e = 0; e < BB; ++e)
            if (R.pick[j * BB + e] != 0.0) fail(t.name, "the padding of the pick covariances");
    }
    for (size_t c = 0; c < C; ++c) {
        for (int q = 0; q < DP; ++q)
            for (int qq = 0; qq < DP; ++qq)
                if (R.remaining[c * BB + q * DP + qq] != R.remaining[c * BB + qq * DP + q]) fail(t.name, "a remaining block is not symmetric");
        if (!t.excluded.empty() && t.excluded[c]) {
            saw_excluded = true;
            for (int32_t p : R.order)
                if (p == (int32_t)c) fail(t.name, "an excluded candidate was picked");
        }
    }
    std::printf("case %s dim %d C %d k %d min_gain %.17g\n", t.name.c_str(), t.dim, (int)t.C, (int)t.k, t.min_gain);
    print_row("P", t.P); print_row("kappa", t.kappa); print_row("tau", t.tau);
    print_row("excluded", t.excluded.empty() ? std::vector<int32_t>(C, 0) : t.excluded);
    std::printf("picked %d\n", (int)got);
    print_row("order", R.order); print_row("gains", R.gains); print_row("pick", R.pick); print_row("remaining", R.remaining);
    return R;
}
Result run(const Table& t, Exit how) {
    reached[how] = true;
    return t.dim == 2 ? run_dp<3>(t) : run_dp<6>(t);
}

// P (N x N) with the DP x DP blocks b[c][d] * I
std::vector<double> scalar_blocks(int C, int DP, const std::vector<double>& b) {
    const size_t N = (size_t)C * DP;
    std::vector<double> P(N * N, 0.0);
    for (int c = 0; c < C; ++c)
        for (int d = 0; d < C; ++d)
            for (int q = 0; q < DP; ++q) P[((size_t)c * DP + q) * N + (size_t)d * DP + q] = b[(size_t)c * C + d];
    return P;
}
// every block of the result is value * I
void expect_block(const std::string& name, const std::vector<double>& blocks, size_t at, int DP, double value) {
    for (int q = 0; q < DP; ++q)
        for (int qq = 0; qq < DP; ++qq)
            if (!close(blocks[at * DP * DP + q * DP + qq], q == qq ? value : 0.0)) fail(name, "block " + std::to_string(at));
}

void refused(const char* what, int32_t C, int dim, int32_t k, double min_gain, const double* kappa, const double* tau) {
    try {
        selp_check(C, dim, k, min_gain, kappa, tau, "check: ");
    } catch (const std::runtime_error& e) {
        if (std::string(e.what()).rfind("check: ", 0) != 0) fail(what, "the message does not start with the caller's name");
        return;
    }
    fail(what, "accepted");
}

}  // namespace

int main() {
    // the gain of a block: 1/2 logdet; a pivot that is not > 0: 0
    {
        const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, D3[9] = {4, 0, 0, 0, 9, 0, 0, 0, 2};
        const double M3[9] = {4, 2, 0, 2, 5, 0, 0, 0, 3};                 // det = (20 - 4) 3 = 48
        const double bad[9] = {1, 2, 0, 2, 1, 0, 0, 0, 1}, neg[9] = {-1, 0, 0, 0, 1, 0, 0, 0, 1}, nan[9] = {NAN, 0, 0, 0, 1, 0, 0, 0, 1};
        if (selp_gain<3>(I3) != 0.0) fail("selp_gain", "the identity");
        if (!close(selp_gain<3>(D3), 0.5 * std::log(72.0))) fail("selp_gain", "a diagonal block");
        if (!close(selp_gain<3>(M3), 0.5 * std::log(48.0))) fail("selp_gain", "a coupled block");
        if (selp_gain<3>(bad) != 0.0 || selp_gain<3>(neg) != 0.0 || selp_gain<3>(nan) != 0.0) fail("selp_gain", "a pivot that is not > 0");
        double I6[36] = {0};
        for (int q = 0; q < 6; ++q) I6[q * 7] = 2.0;
        if (!close(selp_gain<6>(I6), 3.0 * std::log(2.0))) fail("selp_gain", "six pivots");
        if (!selp_stop(0.0, 0.0) || !selp_stop(-1.0, 0.0) || !selp_stop(NAN, 0.0) || selp_stop(0.1, 0.0)) fail("selp_stop", "no gain");
        if (!selp_stop(0.69, 0.7) || selp_stop(0.7, 0.7)) fail("selp_stop", "min_gain");
        const double w3[3] = {4, 1, 9};
        if (selp_scaled<3>(D3, w3, 0, 0) != 0.75 || selp_scaled<3>(D3, w3, 2, 2) != 1.0 / 9.0 || selp_scaled<3>(M3, w3, 0, 1) != 1.0)
            fail("selp_scaled", "the entries");
        // the columns' precisions: 2 tau on the rotation coordinates, kappa on the translations
        const double kap[2] = {3, 5}, ta[2] = {7, 11};
        double w2[6], w6[12];
        selp_weights(2, 2, kap, ta, w2);
        selp_weights(2, 3, kap, ta, w6);
        const double want2[6] = {14, 3, 3, 22, 5, 5}, want6[12] = {14, 14, 14, 3, 3, 3, 22, 22, 22, 5, 5, 5};
        for (int i = 0; i < 6; ++i)
            if (w2[i] != want2[i]) fail("selp_weights", "2-D");
        for (int i = 0; i < 12; ++i)
            if (w6[i] != want6[i]) fail("selp_weights", "3-D");
    }

    // identity, equal precisions (kappa = 4, tau = 2: every w = 4, A = 5 I): index order, equal gains 3/2 log 5
    {
        Result R = run({"identity", 2, 3, 3, 0.0, scalar_blocks(3, 3, {1, 0, 0, 0, 1, 0, 0, 0, 1}), {4, 4, 4}, {2, 2, 2}, {}, 3, {0, 1, 2}}, kAll);
        for (size_t j = 0; j < 3; ++j) {
            if (R.gains[j] != R.gains[0] || !close(R.gains[j], 1.5 * std::log(5.0))) fail("identity", "the gains");
            expect_block("identity", R.pick, j, 3, 1.0);
        }
        saw_tie = true;
    }
    // a duplicated candidate (P blocks all I, w = 4): A = [[5 I, 4 I], [4 I, 5 I]]; 0 first, then B_1 = (5 - 16 / 5) I = 1.8 I
    {
        Result R = run({"duplicate", 2, 2, 2, 0.0, scalar_blocks(2, 3, {1, 1, 1, 1}), {4, 4}, {2, 2}, {}, 2, {0, 1}}, kAll);
        if (!close(R.gains[0], 1.5 * std::log(5.0)) || !close(R.gains[1], 1.5 * std::log(1.8), 16.0) || !(R.gains[1] < R.gains[0]))
            fail("duplicate", "the gains");
        expect_block("duplicate", R.pick, 0, 3, 1.0);
        expect_block("duplicate", R.pick, 1, 3, 0.2);
        // k = 1 of the same: the other's remaining covariance is (1.8 - 1) / 4 I = 0.2 I
        R = run({"duplicate_k1", 2, 2, 1, 0.0, scalar_blocks(2, 3, {1, 1, 1, 1}), {4, 4}, {2, 2}, {}, 1, {0}}, kAll);
        expect_block("duplicate_k1", R.remaining, 0, 3, 1.0);
        expect_block("duplicate_k1", R.remaining, 1, 3, 0.2);
        saw_duplicate = true;
    }
    // the same in 3-D: DP = 6
    {
        Result R = run({"duplicate_3d", 3, 2, 2, 0.0, scalar_blocks(2, 6, {1, 1, 1, 1}), {4, 4}, {2, 2}, {}, 2, {0, 1}}, kAll);
        if (!close(R.gains[0], 3.0 * std::log(5.0)) || !close(R.gains[1], 3.0 * std::log(1.8), 16.0)) fail("duplicate_3d", "the gains");
        expect_block("duplicate_3d", R.pick, 1, 6, 0.2);
    }
    // a zero block (B = I, gain 0) is never picked: the rule stops at it
    {
        Result R = run({"zero_block", 2, 3, 3, 0.0, scalar_blocks(3, 3, {0, 0, 0, 0, 2, 0, 0, 0, 0}), {1, 1, 1}, {0.5, 0.5, 0.5}, {}, 1, {1, -1, -1}}, kNoGain);
        expect_block("zero_block", R.remaining, 0, 3, 0.0);
        expect_block("zero_block", R.remaining, 1, 3, 2.0);
    }
    // the best candidate excluded: never picked, and after the other two nothing is eligible
    {
        Result R = run({"excluded", 2, 3, 3, 0.0, scalar_blocks(3, 3, {2, 0, 0, 0, 8, 0, 0, 0, 1}), {1, 1, 1}, {0.5, 0.5, 0.5}, {0, 1, 0}, 2, {0, 2, -1}}, kNoneEligible);
        expect_block("excluded", R.remaining, 1, 3, 8.0);
    }
    // gains 3/2 log 9 = 3.30, 3/2 log 4 = 2.08, 3/2 log 1.5 = 0.61 against min_gain 1
    {
        Result R = run({"min_gain", 2, 3, 3, 1.0, scalar_blocks(3, 3, {3, 0, 0, 0, 8, 0, 0, 0, 0.5}), {1, 1, 1}, {0.5, 0.5, 0.5}, {}, 2, {1, 0, -1}}, kMinGain);
        if (!close(R.gains[0], 1.5 * std::log(9.0)) || !close(R.gains[1], 1.5 * std::log(4.0))) fail("min_gain", "the gains");
        expect_block("min_gain", R.remaining, 2, 3, 0.5);
    }
    // coupled 2-D candidates with unequal precisions and an asymmetric P: P = M M' / 8 + a small antisymmetric part, M written
    // out; the order is held to the brute-force argmax of 1/2 logdet A_SS pick by pick (run_dp)
    {
        const int N = 9;
        const double M[N][4] = {{2, 1, 0, 1}, {0, 3, 1, 0}, {1, 0, 2, 1}, {2, 1, 1, 1}, {1, 2, 1, 0}, {0, 0, 2, 2}, {1, 1, 1, 3}, {3, 0, 1, 0}, {0, 2, 0, 1}};
        std::vector<double> P((size_t)N * N);
        for (int r = 0; r < N; ++r)
            for (int c = 0; c < N; ++c) {
                double s = 0.0;
                for (int m = 0; m < 4; ++m) s += M[r][m] * M[c][m];
                P[(size_t)r * N + c] = s / 8.0 + (r == c ? 0.25 : 0.0) + (r < c ? 1.0 : r > c ? -1.0 : 0.0) / 1024.0;
            }
        run({"coupled", 2, 3, 3, 0.0, P, {1, 4, 2}, {0.5, 1, 3}, {}, 3, {2, 1, 0}}, kAll);
        run({"coupled_k2", 2, 3, 2, 0.0, P, {1, 4, 2}, {0.5, 1, 3}, {}, 2, {2, 1}}, kAll);
    }
    // and two coupled 3-D candidates
    {
        const int N = 12;
        std::vector<double> P((size_t)N * N);
        for (int r = 0; r < N; ++r)
            for (int c = 0; c < N; ++c) P[(size_t)r * N + c] = (r == c ? 1.0 + 0.125 * r : 0.0) + 0.0625 * (double)((r * 5 + c * 5 + r * c) % 7) / (1.0 + std::abs(r - c));
        run({"coupled_3d", 3, 2, 2, 0.0, P, {2, 1}, {1, 0.5}, {}, 2, {0, 1}}, kAll);
    }

    const double ok[2] = {1.0, 2.0}, zero[2] = {1.0, 0.0}, nan[2] = {NAN, 1.0}, inf[2] = {1.0, INFINITY}, neg[2] = {-1.0, 1.0};
    std::vector<double> many(1366, 1.0);
    refused("C = 0", 0, 2, 1, 0.0, ok, ok);
    refused("C = 1366 in 2-D", 1366, 2, 1, 0.0, many.data(), many.data());
    refused("C = 683 in 3-D", 683, 3, 1, 0.0, many.data(), many.data());
    refused("dim = 4", 2, 4, 1, 0.0, ok, ok);
    refused("k = 0", 2, 2, 0, 0.0, ok, ok);
    refused("k > C", 2, 2, 3, 0.0, ok, ok);
    refused("k = 86 in 2-D", 1365, 2, 86, 0.0, many.data(), many.data());
    refused("k = 43 in 3-D", 682, 3, 43, 0.0, many.data(), many.data());
    refused("min_gain < 0", 2, 2, 1, -1e-9, ok, ok);
    refused("min_gain NaN", 2, 2, 1, NAN, ok, ok);
    refused("no translation precisions", 2, 2, 1, 0.0, nullptr, ok);
    refused("no rotation precisions", 2, 2, 1, 0.0, ok, nullptr);
    for (const double* bad : {zero, nan, inf, neg}) {
        refused("a bad translation precision", 2, 2, 1, 0.0, bad, ok);
        refused("a bad rotation precision", 2, 2, 1, 0.0, ok, bad);
    }
    try {
        selp_check(2, 2, 2, 0.0, ok, ok, "check: ");
        selp_check(1365, 2, 85, 0.0, many.data(), many.data(), "check: ");
        selp_check(682, 3, 42, 0.0, many.data(), many.data(), "check: ");
    } catch (...) {
        fail("selp_check", "refused valid arguments");
    }

    for (int e = 0; e < kExits; ++e)
        if (!reached[e]) fail("coverage", "exit " + std::to_string(e) + " was not reached");
    if (!saw_tie || !saw_excluded || !saw_duplicate) fail("coverage", "the tie, the duplicate or the exclusion was not reached");
    if (failures) return 1;
    std::printf("every branch reached\n");
    return 0;
}

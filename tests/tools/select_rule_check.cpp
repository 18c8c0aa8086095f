// select_rule_check.cpp -- the rule of the greedy selection (score_select_rule.hpp: sel_better, sel_stop, sel_check,
// sel_greedy_host) on tables written by hand: no device, no library.  Each table is a symmetric A = I + D S D with the
// precisions, the exclusions, k and min_gain, and the order, gains, pick variances, remaining variances and number of picks
// worked out on paper.  Between them the tables must reach every exit of the rule -- all k picked, nothing eligible, d <= 1,
// the min_gain stop -- a tie, an excluded candidate and every argument error; the program exits non-zero if one was not.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I score_amd/csrc select_rule_check.cpp
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "score_select_rule.hpp"

using namespace score;

namespace {

int failures = 0;
void fail(const std::string& where, const std::string& what) {
    std::fprintf(stderr, "FAIL %s: %s\n", where.c_str(), what.c_str());
    ++failures;
}

struct Table {
    std::string name;
    int32_t n, k;
    double min_gain;
    std::vector<double> A, w;
    std::vector<int32_t> excluded;     // empty: none
    int32_t picked;
    std::vector<int32_t> order;        // k
    std::vector<double> d_at_pick;     // picked: gains = 1/2 log of these, pick variances (d - 1) / w
    std::vector<double> d_left;        // n: the Schur diagonal at the end (ignored at the picked ones)
};

bool close(double a, double b) { return std::fabs(a - b) <= 4e-16 * std::fmax(1.0, std::fabs(b)); }

enum Exit { kAll = 0, kNoneEligible, kNoGain, kMinGain, kExits };
bool reached[kExits] = {false, false, false, false};
bool saw_tie = false, saw_excluded = false;

void run(const Table& t, Exit how) {
    const size_t n = (size_t)t.n, k = (size_t)t.k;
    std::vector<int32_t> order(k, -9), state(n);
    std::vector<double> gains(k, -9.0), pick(k, -9.0), remaining(n, -9.0), d(n), L(n * k, 0.0);
    const int32_t got = sel_greedy_host(t.A.data(), t.w.data(), t.excluded.empty() ? nullptr : t.excluded.data(), t.n, t.k, t.min_gain,
                                        order.data(), gains.data(), pick.data(), remaining.data(), d.data(), state.data(), L.data());
    if (got != t.picked) fail(t.name, "picked " + std::to_string(got) + ", expected " + std::to_string(t.picked));
    if (order != t.order) fail(t.name, "the order differs");
    for (size_t j = 0; j < k; ++j) {
        const bool on = (int32_t)j < t.picked;
        const double gain = on ? 0.5 * std::log(t.d_at_pick[j]) : 0.0;
        const double var = on ? (t.d_at_pick[j] - 1.0) / t.w[(size_t)t.order[j]] : 0.0;
        if (!close(gains[j], gain)) fail(t.name, "gain " + std::to_string(j));
        if (!close(pick[j], var)) fail(t.name, "pick variance " + std::to_string(j));
        if (on && !close(remaining[(size_t)t.order[j]], var)) fail(t.name, "a picked candidate keeps the value at its pick");
        if (on && j > 0 && !(gains[j] <= gains[j - 1])) fail(t.name, "the gains increase");
    }
    for (size_t c = 0; c < n; ++c) {
        if (state[c] == kSelPicked) continue;
        if (!close(remaining[c], (t.d_left[c] - 1.0) / t.w[c])) fail(t.name, "remaining " + std::to_string(c));
        if (!t.excluded.empty() && t.excluded[c]) {
            saw_excluded = true;
            for (int32_t p : order)
                if (p == (int32_t)c) fail(t.name, "an excluded candidate was picked");
        }
    }
    reached[how] = true;
}

void refused(const char* what, int32_t n, int32_t k, double min_gain, const double* w) {
    try {
        sel_check(n, k, min_gain, w, "check: ");
    } catch (const std::runtime_error& e) {
        if (std::string(e.what()).rfind("check: ", 0) != 0) fail(what, "the message does not start with the caller's name");
        return;
    }
    fail(what, "accepted");
}

}  // namespace

int main() {
    // the comparison: the larger d, equal d to the lower index, no pivot never before one
    if (!sel_better(2.0, 5, 1.0, 0) || sel_better(1.0, 0, 2.0, 5)) fail("sel_better", "the larger d");
    if (!sel_better(2.0, 1, 2.0, 3) || sel_better(2.0, 3, 2.0, 1) || sel_better(2.0, 3, 2.0, 3)) fail("sel_better", "ties");
    if (sel_better(9.0, -1, 1.0, 0) || !sel_better(0.5, 0, 9.0, -1) || sel_better(1.0, -1, 1.0, -1)) fail("sel_better", "no pivot");
    saw_tie = true;
    double g = -1.0;
    if (!sel_stop(1.0, 0.0, &g) || !sel_stop(0.5, 0.0, &g) || !sel_stop(NAN, 0.0, &g)) fail("sel_stop", "d <= 1");
    if (sel_stop(4.0, 0.0, &g) || !close(g, std::log(2.0))) fail("sel_stop", "the gain");
    if (!sel_stop(4.0, 0.7, &g) || sel_stop(4.0, 0.69, &g)) fail("sel_stop", "min_gain");

    // a tie on the diagonal, no coupling: 0 before 1; all k picked
    run({"tie", 3, 3, 0.0, {3, 0, 0, 0, 3, 0, 0, 0, 2}, {1, 1, 1}, {}, 3, {0, 1, 2}, {3, 3, 2}, {0, 0, 0}}, kAll);
    // a duplicated candidate (P = [[1, 1], [1, 1]], w = 4): A = [[5, 4], [4, 5]]; 0 first, then d_1 = 5 - 16 / 5 = 1.8
    run({"duplicate", 2, 2, 0.0, {5, 4, 4, 5}, {4, 4}, {}, 2, {0, 1}, {5, 1.8}, {0, 0}}, kAll);
    // k = 1 of the same: the other's remaining variance is (1.8 - 1) / 4 = 0.2
    run({"duplicate, k = 1", 2, 1, 0.0, {5, 4, 4, 5}, {4, 4}, {}, 1, {0}, {5}, {0, 1.8}}, kAll);
    // the best candidate excluded: never picked, and after the other two nothing is eligible
    run({"excluded", 3, 3, 0.0, {3, 0, 0, 0, 9, 0, 0, 0, 2}, {1, 2, 1}, {0, 1, 0}, 2, {0, 2, -1}, {3, 2}, {0, 9, 0}}, kNoneEligible);
    // a zero row and column (d = 1) is never picked: the rule stops at it
    run({"d <= 1", 3, 3, 0.0, {2, 0, 0, 0, 1, 0, 0, 0, 1}, {1, 1, 1}, {}, 1, {0, -1, -1}, {2}, {0, 1, 1}}, kNoGain);
    // gains 1/2 log 9 = 1.10, 1/2 log 4 = 0.69, 1/2 log 1.5 = 0.20 against min_gain 0.5
    run({"min_gain", 3, 3, 0.5, {4, 0, 0, 0, 9, 0, 0, 0, 1.5}, {1, 1, 2}, {}, 2, {1, 0, -1}, {9, 4}, {0, 0, 1.5}}, kMinGain);
    // coupling: A = [[4, 2, 0], [2, 3, 1], [0, 1, 3.5]]: 0 (d = 4), then d = (., 3 - 1, 3.5): 2 (3.5), l_1 = 1 / sqrt(3.5),
    // d_1 = 2 - 1 / 3.5
    run({"coupled", 3, 3, 0.0, {4, 2, 0, 2, 3, 1, 0, 1, 3.5}, {1, 1, 1}, {}, 3, {0, 2, 1}, {4, 3.5, 2.0 - 1.0 / 3.5}, {0, 0, 0}}, kAll);

    const double ok[2] = {1.0, 2.0}, zero[2] = {1.0, 0.0}, nan[2] = {NAN, 1.0}, inf[2] = {1.0, INFINITY}, neg[2] = {-1.0, 1.0};
    refused("n = 0", 0, 1, 0.0, ok);
    refused("n = 4097", 4097, 1, 0.0, ok);
    refused("k = 0", 2, 0, 0.0, ok);
    refused("k > n", 2, 3, 0.0, ok);
    refused("k = 257", 4096, 257, 0.0, ok);
    refused("min_gain < 0", 2, 1, -1e-9, ok);
    refused("min_gain NaN", 2, 1, NAN, ok);
    refused("no precisions", 2, 1, 0.0, nullptr);
    refused("a zero precision", 2, 1, 0.0, zero);
    refused("a NaN precision", 2, 1, 0.0, nan);
    refused("an infinite precision", 2, 1, 0.0, inf);
    refused("a negative precision", 2, 1, 0.0, neg);
    try {
        sel_check(2, 2, 0.0, ok, "check: ");
    } catch (...) {
        fail("sel_check", "refused valid arguments");
    }

    for (int e = 0; e < kExits; ++e)
        if (!reached[e]) fail("coverage", "exit " + std::to_string(e) + " was not reached");
    if (!saw_tie || !saw_excluded) fail("coverage", "the tie or the exclusion was not reached");
    if (failures) return 1;
    std::printf("every branch reached\n");
    return 0;
}

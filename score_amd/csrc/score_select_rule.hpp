// score_select_rule.hpp -- the rule of the greedy selection of candidate ranges by joint information gain
// (include/score_select.h), stated once and free of HIP: the comparison of two pivots with its tie rule, the stop rule, the
// argument checks, and the whole selection as a plain host routine (sel_greedy_host).  The device kernel k_sel_greedy
// (score_select.hpp) decides with sel_better / sel_stop too; tests/tools/select_rule_check.cpp drives the host routine on tables
// written by hand, and selection.greedy_reference restates it in NumPy.
//
// With S = (P + P')/2, D = diag(sqrt w) and A = I + D S D (symmetric, bit for bit), the selection is a diagonally pivoted
// Cholesky factorisation of A:
//   1. d_c = A_cc.  A candidate is eligible if it is neither picked nor excluded.
//   2. step j: the eligible p with the largest d_p, ties to the lowest index.
//   3. stop if none is eligible, if !(d_p > 1), or if 1/2 log d_p < min_gain.
//   4. order[j] = p, gains[j] = 1/2 log d_p, pick_variances[j] = (d_p - 1) / w_p.
//   5. for EVERY c: l_c = (A_cp - sum_{i<j} L_ci L_pi) / sqrt(d_p), the sum subtracted term by term with i ascending;
//      L_cj = l_c, d_c -= l_c^2.
//   6. after the last pick remaining[c] = (d_c - 1) / w_c of an unpicked candidate; a picked one keeps the value at its pick.
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

#if defined(__HIPCC__)
#define SCORE_SEL_HD __host__ __device__ __forceinline__
#else
#define SCORE_SEL_HD inline
#endif

namespace score {

constexpr int kSelMaxCandidates = 4096;  // P takes 134 MB there
constexpr int kSelMaxPicks = 256;
// the states of a candidate
constexpr int32_t kSelExcluded = 0, kSelEligible = 1, kSelPicked = 2;

// does the pivot (da, ia) come before (db, ib)?  The larger d; equal d: the lower index; index -1: no pivot (never before one).
SCORE_SEL_HD bool sel_better(double da, int32_t ia, double db, int32_t ib) {
    if (ia < 0) return false;
    if (ib < 0) return true;
    return da > db || (da == db && ia < ib);
}
// the selection ends at the pivot d (before it is recorded); *gain = 1/2 log d where it does not
SCORE_SEL_HD bool sel_stop(double d, double min_gain, double* gain) {
    if (!(d > 1.0)) return true;
    *gain = 0.5 * log(d);
    return *gain < min_gain;
}

// the arguments of both entry points
inline void sel_check(int32_t n, int32_t k, double min_gain, const double* precisions, const std::string& who) {
    if (n < 1 || n > kSelMaxCandidates) throw std::runtime_error(who + "the number of candidates must be 1..4096");
    if (k < 1 || k > kSelMaxPicks || k > n) throw std::runtime_error(who + "k must be 1..min(candidates, 256)");
    if (!(min_gain >= 0.0)) throw std::runtime_error(who + "min_gain must be >= 0");
    if (!precisions) throw std::runtime_error(who + "the precisions are missing");
    for (int32_t c = 0; c < n; ++c)
        if (!(precisions[c] > 0.0) || !std::isfinite(precisions[c])) throw std::runtime_error(who + "a precision must be finite and positive");
}

// The selection on the symmetric A (n x n, row-major), w the precisions, excluded (n; null: none): writes order (k, padded with
// -1), gains and pick_variances (k, padded with 0), remaining (n); L: n x k of work, column j at j * n.  Returns the picks.
inline int32_t sel_greedy_host(const double* A, const double* w, const int32_t* excluded, int32_t n, int32_t k, double min_gain,
                               int32_t* order, double* gains, double* pick_variances, double* remaining, double* d, int32_t* state,
                               double* L) {
    for (int32_t c = 0; c < n; ++c) {
        d[c] = A[(size_t)c * n + c];
        state[c] = (excluded && excluded[c]) ? kSelExcluded : kSelEligible;
    }
    int32_t j = 0;
    for (; j < k; ++j) {
        int32_t p = -1;
        double dp = 0.0, gain = 0.0;
        for (int32_t c = 0; c < n; ++c)
            if (state[c] == kSelEligible && sel_better(d[c], c, dp, p)) { dp = d[c]; p = c; }
        if (p < 0 || sel_stop(dp, min_gain, &gain)) break;
        order[j] = p; gains[j] = gain; pick_variances[j] = (dp - 1.0) / w[p];
        remaining[p] = pick_variances[j];
        state[p] = kSelPicked;
        const double root = std::sqrt(dp);
        for (int32_t c = 0; c < n; ++c) {
            double acc = A[(size_t)p * n + c];
            for (int32_t i = 0; i < j; ++i) acc -= L[(size_t)i * n + c] * L[(size_t)i * n + p];
            const double l = acc / root;
            L[(size_t)j * n + c] = l;
            d[c] -= l * l;
        }
    }
    for (int32_t i = j; i < k; ++i) { order[i] = -1; gains[i] = 0.0; pick_variances[i] = 0.0; }
    for (int32_t c = 0; c < n; ++c)
        if (state[c] != kSelPicked) remaining[c] = (d[c] - 1.0) / w[c];
    return j;
}

}  // namespace score

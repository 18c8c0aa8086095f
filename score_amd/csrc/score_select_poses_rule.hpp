// score_select_poses_rule.hpp -- the rule of the greedy selection of candidate loop closures by joint information gain
// (include/score_select_poses.h), stated once and free of HIP: the gain of a candidate's block, the stop rule, the scaling of a
// block to a covariance, the column precisions, the argument checks, and the whole selection as a plain host routine
// (selp_greedy_host).  The device kernel k_selp_greedy (score_select_poses.hpp) decides with selp_gain / sel_better / selp_stop
// too; tests/tools/select_poses_rule_check.cpp drives the host routine on tables written by hand, and
// selection_poses.block_greedy_reference restates it in NumPy.
//
// Candidate c is a relative pose with DP = 3 (2-D) or 6 (3-D) error coordinates, rotation first: its columns are r = c DP + q,
// N = C DP in all, with the precisions w_r = 2 tau_c (q < DP - DIM) and kappa_c (the others) -- relative.measurement_noise.
// With S = (P + P')/2, D = diag(sqrt w) and A = I + D S D (N x N, symmetric bit for bit: k_sel_sym), the gain of a set is
// 1/2 logdet A_SS and the selection is a BLOCK-pivoted Cholesky factorisation of A:
//   1. B_c = the diagonal block of A of candidate c (DP x DP, row-major, symmetric).  Eligible: neither picked nor excluded.
//   2. gain(B) (selp_gain): the unpivoted Cholesky factorisation of B, q ascending: pi_q = B_qq - sum_{m<q} c_qm^2,
//      c_iq = (B_iq - sum_{m<q} c_im c_qm) / sqrt(pi_q) for i > q, every sum subtracted term by term with m ascending.  A pivot
//      that is not > 0: gain 0.  Otherwise s = log pi_0, s += log pi_q with q ascending, gain = 0.5 s.
//   3. step j: the eligible p with the largest gain, ties to the lowest index (sel_better on the gains); stop (selp_stop) if
//      none is eligible, if !(gain_p > 0), or if gain_p < min_gain.
//   4. order[j] = p, gains[j] = gain_p, pick_covariances[j] = selp_scaled(B_p): entry (q, q') is
//      (B_p[q, q'] - [q == q']) / (sqrt w_r * sqrt w_r'), r = p DP + q, r' = p DP + q'.
//   5. DP scalar column steps in fixed order: for q = 0 .. DP - 1, J = j DP + q, r = p DP + q, root = sqrt(B_p[q, q]) with
//      B_p[q, q] as the q earlier sub-steps left it; for EVERY row i
//          l_i = (A[r, i] - sum_{m<J} L[i, m] L[r, m]) / root      (m ascending, term by term),      L[i, J] = l_i,
//      and for every candidate c, p included, and every (q', q''): B_c[q', q''] -= l_{c DP + q'} * l_{c DP + q''} -- formed
//      once for q' >= q'' and stored at both places, so a block stays symmetric bit for bit.
//   6. after the last pick remaining[c] = selp_scaled(B_c) of an unpicked candidate; a picked one keeps the value at its pick.
// What the list leaves open is fixed by the text below and nowhere else: a pick is made only where gain_p > 0, i.e. where the
// block's own factorisation found DP positive pivots; the roots of step 5 are the same numbers up to rounding.
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "score_select_rule.hpp"

namespace score {

// C DP <= kSelMaxCandidates columns of P, k DP <= kSelMaxPicks columns of L
constexpr int selp_dp(int dim) { return dim == 2 ? 3 : 6; }
constexpr int selp_max_candidates(int dp) { return kSelMaxCandidates / dp; }   // 1365, 682
constexpr int selp_max_picks(int dp) { return kSelMaxPicks / dp; }             // 85, 42

// the gain of the block B (DP x DP, row-major; its lower triangle is read)
template <int DP>
SCORE_SEL_HD double selp_gain(const double* B) {
    double c[DP * DP];
    double s = 0.0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int q = 0; q < DP; ++q) {
        double pi = B[q * DP + q];
        for (int m = 0; m < q; ++m) pi -= c[q * DP + m] * c[q * DP + m];
        if (!(pi > 0.0)) return 0.0;
        const double lg = log(pi);
        s = q == 0 ? lg : s + lg;
        const double root = sqrt(pi);
        for (int i = q + 1; i < DP; ++i) {
            double acc = B[i * DP + q];
            for (int m = 0; m < q; ++m) acc -= c[i * DP + m] * c[q * DP + m];
            c[i * DP + q] = acc / root;
        }
    }
    return 0.5 * s;
}
// the selection ends at the gain (before it is recorded)
SCORE_SEL_HD bool selp_stop(double gain, double min_gain) { return !(gain > 0.0) || gain < min_gain; }
// entry (q, q') of the block B of a candidate whose columns have the precisions w (DP of them), as a covariance
template <int DP>
SCORE_SEL_HD double selp_scaled(const double* B, const double* w, int q, int qq) {
    return (B[q * DP + qq] - (q == qq ? 1.0 : 0.0)) / (sqrt(w[q]) * sqrt(w[qq]));
}

// w (C DP): the precisions of the columns from the candidates' kappa (translation) and tau (rotation)
inline void selp_weights(int32_t C, int dim, const double* kappa, const double* tau, double* w) {
    const int DP = selp_dp(dim);
    for (int32_t c = 0; c < C; ++c)
        for (int q = 0; q < DP; ++q) w[(size_t)c * DP + q] = q < DP - dim ? 2.0 * tau[c] : kappa[c];
}

// the arguments of both entry points
inline void selp_check(int32_t C, int dim, int32_t k, double min_gain, const double* kappa, const double* tau, const std::string& who) {
    if (dim != 2 && dim != 3) throw std::runtime_error(who + "dim must be 2 or 3");
    const int DP = selp_dp(dim);
    if (C < 1 || C > selp_max_candidates(DP))
        throw std::runtime_error(who + "the number of candidates must be 1.." + std::to_string(selp_max_candidates(DP)));
    if (k < 1 || k > selp_max_picks(DP) || k > C)
        throw std::runtime_error(who + "k must be 1..min(candidates, " + std::to_string(selp_max_picks(DP)) + ")");
    if (!(min_gain >= 0.0)) throw std::runtime_error(who + "min_gain must be >= 0");
    if (!kappa || !tau) throw std::runtime_error(who + "the precisions are missing");
    for (int32_t c = 0; c < C; ++c)
        if (!(kappa[c] > 0.0) || !std::isfinite(kappa[c]) || !(tau[c] > 0.0) || !std::isfinite(tau[c]))
            throw std::runtime_error(who + "a precision must be finite and positive");
}

// The selection on the symmetric A (N x N, N = C DP, row-major), w (N) the columns' precisions, excluded (C; null: none):
// writes order (k, padded with -1), gains (k, padded with 0), pick_covariances (k DP^2, padded with 0), remaining (C DP^2);
// work: B (C DP^2), state (C), L (N x k DP, column J at J * N).  Returns the picks.
template <int DP>
int32_t selp_greedy_host(const double* A, const double* w, const int32_t* excluded, int32_t C, int32_t k, double min_gain,
                         int32_t* order, double* gains, double* pick_covariances, double* remaining, double* B, int32_t* state,
                         double* L) {
    constexpr int BB = DP * DP;
    const size_t N = (size_t)C * DP;
    for (int32_t c = 0; c < C; ++c) {
        for (int q = 0; q < DP; ++q)
            for (int qq = 0; qq < DP; ++qq) B[(size_t)c * BB + q * DP + qq] = A[((size_t)c * DP + q) * N + (size_t)c * DP + qq];
        state[c] = (excluded && excluded[c]) ? kSelExcluded : kSelEligible;
    }
    int32_t j = 0;
    for (; j < k; ++j) {
        int32_t p = -1;
        double gp = 0.0;
        for (int32_t c = 0; c < C; ++c) {
            if (state[c] != kSelEligible) continue;
            const double g = selp_gain<DP>(B + (size_t)c * BB);
            if (sel_better(g, c, gp, p)) { gp = g; p = c; }
        }
        if (p < 0 || selp_stop(gp, min_gain)) break;
        double* Bp = B + (size_t)p * BB;
        order[j] = p; gains[j] = gp;
        for (int q = 0; q < DP; ++q)
            for (int qq = 0; qq < DP; ++qq)
                remaining[(size_t)p * BB + q * DP + qq] = pick_covariances[(size_t)j * BB + q * DP + qq] =
                    selp_scaled<DP>(Bp, w + (size_t)p * DP, q, qq);
        state[p] = kSelPicked;
        for (int q = 0; q < DP; ++q) {
            const size_t J = (size_t)j * DP + q, r = (size_t)p * DP + q;
            const double root = std::sqrt(Bp[q * DP + q]);
            double* l = L + J * N;
            for (size_t i = 0; i < N; ++i) {
                double acc = A[r * N + i];
                for (size_t m = 0; m < J; ++m) acc -= L[m * N + i] * L[m * N + r];
                l[i] = acc / root;
            }
            for (int32_t c = 0; c < C; ++c)
                for (int a = 0; a < DP; ++a)
                    for (int b = 0; b <= a; ++b) {
                        const double v = B[(size_t)c * BB + a * DP + b] - l[(size_t)c * DP + a] * l[(size_t)c * DP + b];
                        B[(size_t)c * BB + a * DP + b] = B[(size_t)c * BB + b * DP + a] = v;
                    }
        }
    }
    for (int32_t i = j; i < k; ++i) {
        order[i] = -1; gains[i] = 0.0;
        for (int e = 0; e < BB; ++e) pick_covariances[(size_t)i * BB + e] = 0.0;
    }
    for (int32_t c = 0; c < C; ++c)
        if (state[c] != kSelPicked)
            for (int q = 0; q < DP; ++q)
                for (int qq = 0; qq < DP; ++qq)
                    remaining[(size_t)c * BB + q * DP + qq] = selp_scaled<DP>(B + (size_t)c * BB, w + (size_t)c * DP, q, qq);
    return j;
}

}  // namespace score

/*
 * score_select.h -- greedy selection of candidate ranges by joint information gain at a refined estimate (HIP library only,
 * like score_leverage.h).
 *
 * score_refine_range_variances says what ONE hypothetical range would be worth: 1/2 log(1 + w g'H^-1 g).  The gains of
 * several candidates do not add: two candidates at neighbouring poses are nearly the same measurement.  For the Gaussian
 * posterior at the estimate, adding the set S of ranges with precisions w_c gains
 *     gain(S) = 1/2 [logdet(H + sum_{c in S} w_c g_c g_c') - logdet H] = 1/2 logdet(I + D_S P_SS D_S),
 *     P = G'H^-1 G,  D = diag(sqrt w),
 * which is monotone and submodular, so the greedy rule -- pick the candidate with the largest gain given the picks so far --
 * is within 1 - 1/e of the best set of its size.  That rule is a diagonally pivoted Cholesky factorisation of
 * A = I + D (P + P')/2 D: the Schur-complement diagonal after the picks S is d_c = 1 + w_c sigma^2_{c|S}, with
 * sigma^2_{c|S} = g_c'(H + G_S W_S G_S')^-1 g_c the variance of candidate c once the picks are measured, and the increment of
 * the next pick p is 1/2 log d_p.
 *
 * The rule: eligible = neither picked nor excluded; step j takes the eligible p with the largest d_p, ties to the lowest
 * index; it stops when nothing is eligible, when !(d_p > 1), or when 1/2 log d_p < min_gain; then every d_c loses l_c^2 with
 * l_c = (A_cp - sum_{i<j} L_ci L_pi) / sqrt(d_p).  All in fp64, fixed-order sums, no atomics: two calls give the same bits.
 */
#ifndef SCORE_SELECT_H
#define SCORE_SELECT_H

#include <stdint.h>

#include "score_hip.h"
#include "score_marginals.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct score_select_info {
    score_marginals_info solve;      /* the block PCG, as score_refine_range_variances reports it */
    int32_t candidates, picked, excluded;
    double  total_gain;              /* sum of gains, nats */
    double  asymmetry;               /* max |P_cd - P_dc| as computed */
    double  cross_ms, greedy_ms;
} score_select_info;

/* The columns x_c = H^-1 g_c of score_refine_range_variances on the same pairs, point, rel_tol, max_iters and block_width
 * (variances, distances, residuals, iters: that call's, bit for bit), the cross terms P[c * n_pairs + d] = g_c' x_d after
 * every solved block (column d of P is "as computed", its diagonal is `variances`), and the rule above on them.
 * pair_a / pair_b: as in score_leverage.h (duplicate pairs are allowed); precisions: n_pairs, finite and positive;
 * 1 <= k <= min(n_pairs, 256); n_pairs <= 4096; min_gain >= 0.
 * order: k, the picks in their order, padded with -1.  gains: k, 1/2 log d_p in nats (padding: 0).  pick_variances: k,
 *   (d_p - 1) / w_p: the variance of the pick given the picks before it.
 * remaining: n_pairs, (d_c - 1) / w_c after the last pick; a picked candidate has the value at its own pick.
 * matrix: n_pairs^2, P as computed (normally NULL).
 * A column that did not converge excludes its candidate: it is never picked and info.excluded counts it.
 * Any output may be NULL.  Returns 0; 1: some column did not converge (outputs still written); < 0: error
 * (score_last_error()). */
int score_refine_select_ranges(score_refine* r, const double* poses, const double* landmarks,
                               const int32_t* pair_a, const int32_t* pair_b, const double* precisions, int32_t n_pairs,
                               int32_t k, double min_gain, double rel_tol, int32_t max_iters, int32_t block_width,
                               int32_t* order, double* gains, double* pick_variances,
                               double* variances, double* distances, double* remaining,
                               double* residuals, int32_t* iters, double* matrix,
                               score_select_info* info);

/* The selection alone on a caller's matrix (n x n, row-major; it need not be symmetric: (P + P')/2 is used), no handle, on
 * device 0.  excluded: n, non-zero = never picked (NULL: none).  picked: the number of picks; asymmetry: max |P_cd - P_dc|.
 * Any output may be NULL.  Returns 0; < 0: error. */
int score_select_greedy(const double* matrix, const double* precisions, const int32_t* excluded, int32_t n,
                        int32_t k, double min_gain,
                        int32_t* order, double* gains, double* pick_variances, double* remaining,
                        int32_t* picked, double* asymmetry);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_SELECT_H */

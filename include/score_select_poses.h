/*
 * score_select_poses.h -- greedy selection of candidate loop closures (relative poses) by joint information gain at a refined
 * estimate (HIP library only, like score_select.h).
 *
 * score_refine_relative_covariances says what ONE hypothetical relative pose would be worth: 1/2 logdet(I + N^-1 P_c) with
 * P_c = G_c H^-1 G_c' and N = diag(I / (2 tau), I / kappa).  The gains of several candidates do not add: ten candidate
 * matches between two passes through one corridor are nearly one measurement.  For the Gaussian posterior at the estimate,
 * adding the set S of relative poses gains
 *     gain(S) = 1/2 [logdet(H + sum_{c in S} G_c' N_c^-1 G_c) - logdet H] = 1/2 logdet A_SS,
 *     A = I + D (P + P')/2 D,  P = G H^-1 G' (N x N, N = C DP columns r = c DP + q),  D = diag(sqrt w),
 *     w_r = 2 tau_c for the rotation coordinates (q < DP - DIM), kappa_c for the translation coordinates,
 * monotone and submodular as in the scalar case, so the greedy rule is within 1 - 1/e of the best set of its size.  A
 * candidate is a BLOCK of DP = 3 (2-D) or 6 (3-D) columns: the rule is a block-pivoted Cholesky factorisation of A, the pivot
 * a DP x DP Schur block B_c = I + D_c Sigma_{c|S} D_c scored by gain(B_c) = 1/2 logdet B_c.
 *
 * The rule (csrc/score_select_poses_rule.hpp states it in full): eligible = neither picked nor excluded; step j takes the
 * eligible p with the largest gain(B_p), ties to the lowest index; it stops when nothing is eligible, when !(gain > 0), or
 * when gain < min_gain; then DP scalar column steps of the factorisation, q ascending, update every B_c.  All in fp64,
 * fixed-order sums, no atomics: two calls give the same bits.
 */
#ifndef SCORE_SELECT_POSES_H
#define SCORE_SELECT_POSES_H

#include <stdint.h>

#include "score_hip.h"
#include "score_marginals.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct score_select_poses_info {
    score_marginals_info solve;      /* the block PCG, as score_refine_relative_covariances reports it */
    int32_t candidates, picked, excluded;
    double  total_gain;              /* sum of gains, nats */
    double  asymmetry;               /* max |P_rs - P_sr| as computed */
    double  cross_ms, greedy_ms;
} score_select_poses_info;

/* The columns H x = G_c'e_q of score_refine_relative_covariances on the same pairs, point, rel_tol, max_iters and block_width
 * (rotations, translations, covariances, residuals, iters: that call's, bit for bit), the cross terms
 * P[(c DP + q') N + j] = (G_c x_j)[q'] after every solved block (column j of P is "as computed", its diagonal blocks are
 * `covariances`), and the rule above on them.
 * pair_a / pair_b: as in score_relative.h (duplicate pairs are allowed); translation_precisions (kappa) and
 * rotation_precisions (tau): n_pairs each, finite and positive; with DP = 3 or 6: n_pairs DP <= 4096,
 * 1 <= k <= min(n_pairs, 256 / DP); min_gain >= 0.
 * order: k, the picks in their order, padded with -1.  gains: k, nats (padding: 0).  pick_covariances: k x DP x DP, the
 *   covariance of the pick's error coordinates given the picks before it (padding: 0).
 * remaining: n_pairs x DP x DP, the covariance after the last pick; a picked candidate has the value at its own pick.
 * matrix: (n_pairs DP)^2, P as computed (normally NULL).
 * A candidate with ANY column that did not converge is excluded: it is never picked and info.excluded counts it.
 * Any output may be NULL.  Returns 0; 1: some column did not converge (outputs still written); < 0: error
 * (score_last_error()). */
int score_refine_select_relative_poses(score_refine* r, const double* poses, const double* landmarks,
                                       const int32_t* pair_a, const int32_t* pair_b,
                                       const double* translation_precisions, const double* rotation_precisions,
                                       int32_t n_pairs, int32_t k, double min_gain,
                                       double rel_tol, int32_t max_iters, int32_t block_width,
                                       int32_t* order, double* gains, double* pick_covariances,
                                       double* rotations, double* translations, double* covariances, double* remaining,
                                       double* residuals, int32_t* iters, double* matrix,
                                       score_select_poses_info* info);

/* The selection alone on a caller's matrix (N x N, N = n_candidates DP, row-major; it need not be symmetric: (P + P')/2 is
 * used), no handle, on device 0.  dim: 2 or 3.  excluded: n_candidates, non-zero = never picked (NULL: none).  picked: the
 * number of picks; asymmetry: max |P_rs - P_sr|.  Any output may be NULL.  Returns 0; < 0: error. */
int score_select_block_greedy(const double* matrix, const double* translation_precisions, const double* rotation_precisions,
                              const int32_t* excluded, int32_t n_candidates, int32_t dim, int32_t k, double min_gain,
                              int32_t* order, double* gains, double* pick_covariances, double* remaining,
                              int32_t* picked, double* asymmetry);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_SELECT_POSES_H */

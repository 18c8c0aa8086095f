/*
 * score_leverage.h -- leverage of the measurements and predicted range variances at a refined estimate (HIP library only,
 * like score_samples.h).
 *
 * At a point of a refinement handle, with J the whitened Jacobian and H = J'J (include/score_samples.h), the hat matrix
 * P = J H^-1 J' projects the measurement space onto the range of J.  The leverage of measurement m is
 * h_m = trace(J_m H^-1 J_m') over its rows, 1 - h_m per row its redundancy: a residual shows the share 1 - h_m of an error
 * in its own measurement, and sum_m h_m = n, sum_m (rows_m - h_m) = rows - n.
 *
 * Both come from the posterior draws: with delta = H^-1 J'z and z ~ N(0, I), J delta = P z, so over the rows q of m
 *     E sum_q (J_m delta)_q^2 = h_m,        E sum_q (z - J_m delta)_q^2 = rows_m - h_m.
 * The first has relative error sqrt(2 / S) on h_m, the second on the redundancy: a measurement nothing else controls
 * (h_m = rows_m) gets a redundancy estimate of rounding size from the second, which the first cannot give.
 *
 * The predicted variance of a range between two variables a and b is g' H^-1 g with g the gradient of |p_a - p_b| in the
 * refinement's unknowns: +u on the translation unknowns of a, -u on those of b, u the unit vector of p_a - p_b at the point
 * (zero where |p_a - p_b| <= 1e-12, as in a range measurement's Jacobian; a pose without unknowns -- pose 0 -- contributes
 * nothing).  score_refine_leverage estimates it from the draws, score_refine_range_variances solves H x = g.
 */
#ifndef SCORE_LEVERAGE_H
#define SCORE_LEVERAGE_H

#include <stdint.h>

#include "score_hip.h"
#include "score_marginals.h"
#include "score_samples.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The draws are those of the score_refine_samples call with the same seed, first_sample, n_samples and block_width, bit for
 * bit: the noise stream, the probe column, the stopping rule, the breakdown words, and a failed probe marks every draw as
 * not converged.  poses / landmarks, rel_tol, max_iters, block_width, residuals, iters, info and the return code: as there.
 * Measurements m = 0 .. M - 1, M = n_rel + n_rng + n_pri, numbered as in score_samples.h.  With y = J_m delta_s, z the
 * noise of (m, s), t = sum_q y_q^2 and v = sum_q (z_q - y_q)^2 over the rows q of m:
 * lev_sum, lev_sq: M each, the SUMS over the converged draws, ascending s, of t and of t^2 (not divided by their number);
 * red_sum, red_sq: M each, the same sums of v and v^2.
 * pair_a / pair_b / n_pairs: hypothetical ranges between variable ids as in score_graph's range endpoints (0..Np-1 poses,
 *   Np.. landmarks); a == b: error; an id out of range: error; n_pairs < 0: error; n_pairs may be 0.
 * pair_sum, pair_sq: n_pairs each, the same sums of (g_c' delta_s)^2 and of its square: a range of precision 1 (metres^2).
 * No sum depends on block_width.  Any output may be NULL. */
int score_refine_leverage(score_refine* r, const double* poses, const double* landmarks,
                          uint64_t seed, int64_t first_sample, int32_t n_samples,
                          const int32_t* pair_a, const int32_t* pair_b, int32_t n_pairs,
                          double rel_tol, int32_t max_iters, int32_t block_width,
                          double* lev_sum, double* lev_sq, double* red_sum, double* red_sq,
                          double* pair_sum, double* pair_sq,
                          double* residuals, int32_t* iters,
                          score_samples_info* info);

/* For every pair H x_c = g_c, up to block_width (1..16) pairs per block, by the lock-step iteration of
 * score_refine_marginals (same stopping rule and breakdown words).
 * variances: n_pairs, g_c' x_c.  distances: n_pairs, |p_a - p_b| at the point.
 * residuals: n_pairs, the true residual |g_c - H x_c|_2 from one more product.  iters: n_pairs, the steps a column took --
 *   as -(steps + 1) where it did not converge.
 * solutions: n_pairs x n, x_c as computed (a diagnostic: what the variance and the residual were formed from; normally NULL).
 * Any output may be NULL.  info: columns = n_pairs.
 * Returns 0: all columns converged; 1: some did not (outputs still written); < 0: error (score_last_error()). */
int score_refine_range_variances(score_refine* r, const double* poses, const double* landmarks,
                                 const int32_t* pair_a, const int32_t* pair_b, int32_t n_pairs,
                                 double rel_tol, int32_t max_iters, int32_t block_width,
                                 double* variances, double* distances, double* residuals, int32_t* iters,
                                 double* solutions,
                                 score_marginals_info* info);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_LEVERAGE_H */

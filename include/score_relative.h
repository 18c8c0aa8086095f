/*
 * score_relative.h -- predicted relative poses between pairs of poses and their covariances at a refined estimate (HIP
 * library only, like score_leverage.h): what a Mahalanobis gate in front of a loop closure asks for.
 *
 * DIM is 2 or 3, DP 3 or 6.  The unknowns of a pose and the retraction are those of include/score_marginals.h: 2-D
 * (theta, x, y), additive; 3-D (omega, v) with R Exp(omega), t + v; pose 0 has no unknowns.  For a pair (a, b) of POSES,
 * a != b, either of which may be pose 0:
 *   prediction          R_ab = R_a' R_b,  t_ab = R_a' (t_b - t_a)            (T_a^-1 T_b)
 *   error coordinates   xi (DP), rotation first like the unknowns:
 *                         2-D  xi -> (theta_ab + xi_0, t_ab + xi_1:2),  theta_ab = theta_b - theta_a
 *                         3-D  xi -> (R_ab Exp(xi_0:2), t_ab + xi_3:5)
 *   G (DP x 2 DP)       the derivative of xi in [unknowns of a | unknowns of b] at zero step; the columns of pose 0 are left
 *                       out.  With S = [[0, -1], [1, 0]]:
 *                         2-D  rotation row:     -1 at theta_a, +1 at theta_b
 *                              translation rows: -S t_ab at theta_a, -R_a' at (x_a, y_a), +R_a' at (x_b, y_b)
 *                         3-D  rotation rows:    -R_ab' at omega_a, I at omega_b
 *                              translation rows: [t_ab]x at omega_a, -R_a' at v_a, +R_a' at v_b
 *   covariance          P_c = G_c H^-1 G_c', H = J'J at the point under the handle's current precisions.
 * Column j = c DP + q solves H x_j = G_c' e_q, and P_c[q', q] = (G_c x_j)[q']: DP columns per pair where the joint marginal of
 * both ends (score_refine_marginals) takes 2 DP.
 */
#ifndef SCORE_RELATIVE_H
#define SCORE_RELATIVE_H

#include <stdint.h>

#include "score_hip.h"
#include "score_marginals.h"

#ifdef __cplusplus
extern "C" {
#endif

/* poses / landmarks: the point, laid out as score_refine_run's inputs.
 * pair_a / pair_b / n_pairs: pose ids 0..Np-1.  a == b: error; an id < 0 or >= Np (a landmark): error; n_pairs < 0: error;
 *   pairs without their lists: error; n_pairs == 0: returns 0 and launches nothing.
 * block_width: 1..16 CONSECUTIVE columns per block of the lock-step iteration of score_refine_marginals (same stopping rule
 *   and breakdown words), so a pair may straddle two blocks; every output entry depends on its own column only.
 * rotations: n_pairs x DIM x DIM row-major, R_ab.  translations: n_pairs x DIM, t_ab.
 * covariances: n_pairs x DP x DP row-major, column q as computed (not symmetrised, like joint of score_refine_marginals).
 * residuals: n_pairs x DP, the true residual |G_c'e_q - H x_j|_2 from one more product.
 * iters: n_pairs x DP, the steps a column took -- as -(steps + 1) where it did not converge.
 * solutions: n_pairs*DP x n, x_j as computed (a diagnostic: what P and the residual were formed from; normally NULL).
 * Any output may be NULL.  info: columns = n_pairs*DP, batches = ceil(columns / block_width).
 * Returns 0: all columns converged; 1: some did not (outputs still written); < 0: error (score_last_error()). */
int score_refine_relative_covariances(score_refine* r, const double* poses, const double* landmarks,
                                      const int32_t* pair_a, const int32_t* pair_b, int32_t n_pairs,
                                      double rel_tol, int32_t max_iters, int32_t block_width,
                                      double* rotations, double* translations, double* covariances,
                                      double* residuals, int32_t* iters, double* solutions,
                                      score_marginals_info* info);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_RELATIVE_H */

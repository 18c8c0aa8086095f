/*
 * score_curvature.h -- the second-order check of a refined estimate (HIP library only, like score_spectrum.h).
 *
 * The analyses of include/score_marginals.h, score_spectrum.h, score_samples.h and score_leverage.h read the Gauss-Newton
 * matrix H = J'J, which is positive semidefinite at every point: none of them can tell whether the point a local solver
 * stopped at is a minimum.  Half the Hessian of the cost F = r'r is
 *   E = J'J + sum_q r_q grad^2 r_q          (q over the whitened residual rows),
 * in the refinement's own unknowns (3-D: in the coordinates of the retraction R Exp(omega), t + v).  It lives on the pattern
 * of J'J.  A negative eigenvalue of E is a direction along which the cost falls to second order: the point is a saddle, and
 * the eigenvector says which variables to move.  At a minimum E is the observed information, which differs from J'J where
 * the residuals are not small.
 * The eigenpairs come from the iteration of score_refine_spectrum on A = E + sigma I, sigma = shift_rel * max diag J'J, with
 * the preconditioner of J'J + sigma I (chain factors of an indefinite matrix need not exist).
 */
#ifndef SCORE_CURVATURE_H
#define SCORE_CURVATURE_H

#include <stdint.h>

#include "score_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct score_curvature_info {
    int32_t modes, block, iterations, unconverged;
    double  h_max, shift, c_max, max_residual, setup_ms, solve_ms;   /* h_max: max diag J'J; c_max: max |E - J'J| entry */
} score_curvature_info;

/* out = A V, A = E (exact != 0) or J'J (exact == 0) at the point, no shift.  V, out: n_cols x n row-major, n_cols 1..16. */
int score_refine_hessian_product(score_refine* r, const double* poses, const double* landmarks, int32_t exact,
                                 const double* V, int32_t n_cols, double* out);

/* The k (1..16) lowest eigenpairs of E; arguments, outputs, stopping rule (|E v - lambda v|_2 <= rel_tol * h_max) and return
 * codes as score_refine_spectrum.  gn_quotients: k, v_j'(J'J)v_j.  Values may be negative. */
int score_refine_curvature(score_refine* r, const double* poses, const double* landmarks, int32_t k,
                           double rel_tol, int32_t max_iters, double shift_rel,
                           double* values, double* vectors, double* residuals, double* gn_quotients,
                           score_curvature_info* info);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_CURVATURE_H */

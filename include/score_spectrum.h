/*
 * score_spectrum.h -- the weakest modes of a refined estimate (HIP library only, like score_marginals.h).
 *
 * At a point (poses, landmarks) of a refinement handle (score_refine_create, include/score_hip.h) the Gauss-Newton matrix
 * H = J'J is the information matrix of the estimate in the refinement's own unknowns (include/score_marginals.h).  Its
 * lowest eigenpairs say which combination of variables the measurements determine least -- an eigenvalue at zero: not at
 * all -- and bracket every marginal covariance at once: with the lowest m pairs (lambda_j, v_j),
 *   L = sum_{j < m-1} v_j v_j' / lambda_j   and   L_vv <= Sigma_vv <= L_vv + I / lambda_{m-1}   for every variable v.
 * The call runs LOBPCG (Knyazev 2001) with a block of 16 vectors on A = H + sigma I, sigma = shift_rel * max diag H, with
 * the chain preconditioner of score_refine_marginals; the shift is what lets the chain factors exist when H is singular.
 */
#ifndef SCORE_SPECTRUM_H
#define SCORE_SPECTRUM_H

#include <stdint.h>

#include "score_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct score_spectrum_info {
    int32_t modes, block, iterations, unconverged;   /* k asked, vectors iterated (16), LOBPCG iterations, pairs above tolerance */
    double  h_max, shift, max_residual;              /* max diag H; sigma = shift_rel * h_max as used; largest |H v - lambda v|_2 */
    double  setup_ms, solve_ms;
} score_spectrum_info;

/* The k (1..16) lowest eigenpairs of H = J'J at (poses, landmarks) of a refinement handle; the unknowns and their order
 * are score_refine_marginals' (pose 0 fixed).  values: k ascending.  vectors: k x n row-major, unit 2-norm.
 * residuals: k, |H v - lambda v|_2 from one more product after the iteration.  Any output may be NULL.
 * Returns 0: all k pairs reached rel_tol * h_max; 1: some did not (outputs still written); < 0: error. */
int score_refine_spectrum(score_refine* r, const double* poses, const double* landmarks, int32_t k,
                          double rel_tol, int32_t max_iters, double shift_rel,
                          double* values, double* vectors, double* residuals, score_spectrum_info* info);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_SPECTRUM_H */

/*
 * score_marginals.h -- marginal covariances of a refined estimate (HIP library only, like score_robust.h).
 *
 * At a point (poses, landmarks) of a refinement handle (score_refine_create, include/score_hip.h) the Gauss-Newton matrix
 * H = J'J of the maximum-likelihood cost is the information matrix of the estimate in the refinement's own unknowns; the
 * covariance of a set S of variables is the S x S part of H^-1.  The call solves H X = E_S -- one unit column per scalar
 * unknown of S -- on the device: H is gathered on the handle's fixed pattern, its pose chains are factored once, and a
 * chain-preconditioned conjugate-gradient iteration advances a block of up to 16 columns in lock-step (one pass over H
 * per iteration for the whole block).  Every column stops on the rule of score_linear_solve,
 *   r'M^-1 r <= rel_tol^2 r0'M^-1 r0,
 * and reports its true residual |e_c - H x_c|_2, computed with one more product after the block has finished.
 */
#ifndef SCORE_MARGINALS_H
#define SCORE_MARGINALS_H

#include <stdint.h>

#include "score_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct score_marginals_info {
    int32_t columns;       /* C: scalar unknowns of the selected variables                                         */
    int32_t batches;       /* blocks of columns solved (block_width = 0: C single solves)                          */
    int32_t pcg_iters;     /* iterations queued and executed: per block the most any of its columns took, summed   */
    int32_t unconverged;   /* columns that hit max_iters or broke down (non-finite r'z or p'w, p'w <= 0)           */
    double  max_residual;  /* largest |e_c - H x_c|_2                                                              */
    double  setup_ms;      /* blocks at the point, H, chain factors, buffers                                       */
    double  solve_ms;      /* the solves, residuals and the copy back                                              */
} score_marginals_info;

/* poses / landmarks: the point, laid out as score_refine_run's inputs.
 * vars: variable ids as in score_graph's range endpoints (0..Np-1 poses, Np.. landmarks).
 * Pose 0 is fixed: error.  Duplicates: error.
 * Columns per variable, in this order:
 *   2-D pose (theta, x, y); 2-D landmark (x, y);
 *   3-D pose (omega, v) of the retraction R Exp(omega), t + v; 3-D landmark (x, y, z).
 * block_width: 1..16 columns per block; 0: one column at a time through the single-right-hand-side solve of
 *   score_linear_solve (the loop-closure correction of its preconditioner included).
 * joint: C x C row-major, column c as computed (not symmetrised).
 * residuals: C.  iters: C, the steps a column took -- as -(steps + 1) where it did not converge.  Any output may be NULL.
 * Returns 0: all columns converged; 1: some did not (outputs still written); < 0: error (score_last_error()). */
int score_refine_marginals(score_refine* r, const double* poses, const double* landmarks,
                           const int32_t* vars, int32_t n_vars,
                           double rel_tol, int32_t max_iters, int32_t block_width,
                           double* joint, double* residuals, int32_t* iters,
                           score_marginals_info* info);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_MARGINALS_H */

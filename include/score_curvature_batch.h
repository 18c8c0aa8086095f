/*
 * score_curvature_batch.h -- the second-order check of EVERY member of a refinement group (HIP library only, like
 * score_spectrum_batch.h).
 *
 * score_refine_curvature (include/score_curvature.h) gives the lowest eigenpairs of E = J'J + sum_q r_q grad^2 r_q, half the
 * Hessian of the cost, of one graph per handle, and reads a 48 x 48 pencil back to the host in every iteration.  "Did this
 * world's refinement stop at a minimum or at a saddle?" is asked of all the worlds of a study.  A group handle
 * (score_refine_batch_create, include/score_refine_batch.h) holds them as ONE union problem; E_g lives on member g's part of
 * the union pattern, so the lock-step rounds of score_refine_batch_spectrum (include/score_spectrum_batch.h) carry it as they
 * are: the product reads E_g + sigma_g I from a value array of the call's own, the Rayleigh-Ritz kernel lets the lowest
 * value be negative, and the preconditioner stays that of J'J + sigma_g I (chain factors of an indefinite matrix need not
 * exist).
 *
 * Per member g the contract is that of score_curvature.h: sigma_g = shift_rel * h_max_g (h_max_g = max diag J'J of the
 * member), a pair counts as converged at |E_g v - lambda v|_2 <= rel_tol * h_max_g, a member ends only on the residuals of a
 * true product.  Members never influence one another: a member's outputs are those of a group that holds it alone, bit for
 * bit, and two calls give the same bits.
 *
 * Memory: the 16-vector blocks are those of score_refine_batch_spectrum (allocated once per handle whichever call comes
 * first); beside them the exact block storage, one value array on the union pattern and a few partials.
 *
 * Both calls leave the handle as they found it: a later score_refine_batch_run or score_refine_batch_spectrum equals a fresh
 * handle's, bit for bit.
 */
#ifndef SCORE_CURVATURE_BATCH_H
#define SCORE_CURVATURE_BATCH_H

#include <stdint.h>

#include "score_refine_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct score_curvature_batch_info {
    int32_t members;       /* members of the group                                                                 */
    int32_t modes;         /* k asked of every member                                                              */
    int32_t block;         /* vectors iterated per member (16)                                                     */
    int32_t rounds;        /* lock-step passes queued                                                              */
    int32_t unconverged;   /* members with a pair above tolerance (or broken down)                                 */
    int32_t saddles;       /* members with a value < -rel_tol * h_max_g                                            */
    double  max_residual;  /* largest |E_g v - lambda v|_2 of the call                                             */
    double  setup_ms;      /* blocks at the points, J'J, max diag, chain factors, exact blocks, E, c_max, buffers  */
    double  solve_ms;      /* the rounds, the Gauss-Newton product and the copy back                               */
} score_curvature_batch_info;

/* out_g = A_g V_g for every member, A = E (exact != 0) or J'J (exact == 0) at the points, no shift.  poses / landmarks: the
 * members' points one after the other, laid out as score_refine_batch_run's inputs.  Member g: V_g and out_g are
 * n_cols x n_g row-major, the members one after the other; n_cols 1..16.  Fewer columns give the bits of the same columns
 * at 16.  Returns 0, or < 0: error (score_last_error()). */
int score_refine_batch_hessian_product(score_refine_batch* b, const double* poses, const double* landmarks, int32_t exact,
                                       const double* V, int32_t n_cols, double* out);

/* The k (1..16) lowest eigenpairs of E_g of every member.  Arguments, layout, stopping rule, iteration encoding and return
 * codes as score_refine_batch_spectrum: values count x k ascending per member (they may be negative), vectors k x n_g
 * row-major per member, residuals count x k, iterations count (as -(it + 1) where not all k pairs converged), h_max count
 * (max diag J'J).  gn_quotients: count x k, v_j'(J'J)v_j beside every value; c_max: count, the largest |E_g - J'J| entry.
 * Any output may be NULL.  A member with fewer than 48 unknowns: error naming the member. */
int score_refine_batch_curvature(score_refine_batch* b, const double* poses, const double* landmarks, int32_t k,
                                 double rel_tol, int32_t max_iters, double shift_rel,
                                 double* values, double* vectors, double* residuals, double* gn_quotients,
                                 int32_t* iterations, double* h_max, double* c_max, score_curvature_batch_info* info);

/* score_spectrum_ritz (include/score_spectrum_batch.h) with the indefinite rule (no handle; device 0): the test that the
 * lowest Ritz value is positive is lifted, nothing else -- S'S must still be positive definite on the directions kept.  The
 * pencil of a positive definite operator gives the bits score_spectrum_ritz gives. */
int score_curvature_ritz(int32_t count, const double* GA, const double* GB, double* theta, double* coef,
                         int32_t* status, int32_t* kept);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_CURVATURE_BATCH_H */

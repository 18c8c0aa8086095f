/*
 * score_refine_robust.h -- outlier-robust local refinement (HIP library only, like score_marginals.h): GNC-TLS re-weighting of
 * the range measurements and / or the loop closures on the residuals of the maximum-likelihood cost, the whole outer loop on
 * one refinement handle (score_refine_create, include/score_hip.h), in 2-D and 3-D.
 *
 * The relaxation's robust loop (include/score_robust.h) weighs a range by its term in the RELAXED objective: a range measured
 * too long costs nothing there and keeps weight 1.  The refinement's range term w (|p_a - p_b| - dist)^2 is two-sided, so this
 * loop sees it.  Families and the single mu per graph are those of score_robust.h; the residuals and the solve differ.
 *
 * Residuals, at the current point (poses on the manifold, landmarks) with the MEASURED precisions, never the weighted ones:
 *   range         r = sqrt(prec) | |p_a - p_b| - dist |                                              (two-sided)
 *   loop closure  r = sqrt( kappa |t_j - t_i - R_i t~|^2 + tau |R_j - R_i R~|_F^2 )
 *                 -- the square root of the relative-pose term of the refinement's cost (R = R(theta) in 2-D; pose 0 is where
 *                 the caller put it).  The loop closures are the trailing n_rel - sum(chain_len - 1) relative-pose entries.
 * Both are the square root of what the refinement's own block functions cost (csrc/score_gn.hpp: gn_robust_residual<DIM>).
 *
 * The loop (enabled families f: ranges c_f = inlier_threshold, loop closures c_f = rel_threshold):
 *   1. weights w = 1; solve 1 is the Levenberg-Marquardt loop exactly as score_refine_run runs it (max_iters, tol);
 *   2. after a solve: the residuals of the enabled families; stop if
 *        - it was solve 1 and no enabled family has 2 max r_f^2 > c_f^2: the result IS score_refine_run's, bit for bit, with
 *          outer_iterations = 1 and converged = 1;
 *        - a later solve ran on weights that are binary (within 1e-6 of 0 or 1) in every enabled family: converged = 1;
 *        - max_outer solves are done: converged = 0;
 *        - a residual is non-finite: converged = 0;
 *   3. otherwise mu = min over the families with 2 max r_f^2 > c_f^2 of c_f^2 / (2 max r_f^2 - c_f^2) after solve 1,
 *      mu <- mu_step * mu after later solves;
 *        w = 1 if r^2 <= mu / (mu + 1) c_f^2,   w = 0 if r^2 >= (mu + 1) / mu c_f^2,   w = c_f / r sqrt(mu (mu + 1)) - mu otherwise;
 *      the next solve's precisions are prec * max(w, min_weight); a loop closure scales kappa and tau together;
 *   4. solves 2, 3, ... are Levenberg-Marquardt from the current point, at most inner_iters iterations each;
 *   5. when the loop stops after a later solve (on finite residuals), one last Levenberg-Marquardt run with the final weights goes
 *      to max_iters / tol: the reported estimate, cost and gradient are that run's.  The reported residuals are taken at the
 *      final estimate.
 * An enabled family without measurements takes no part (no launch); if every enabled family is empty the loop stops after solve 1.
 *
 * The handle keeps the measured precisions in device arrays of their own.  Residuals and weights are computed by two
 * kernels at the point on the device; one device-to-host read per outer iteration (per-block maxima of r^2 and counts of
 * non-binary weights) steers the loop.  On return -- an error return included -- the handle holds the measured precisions
 * again: a later score_refine_run or score_refine_marginals on it equals a fresh handle's.
 */
#ifndef SCORE_REFINE_ROBUST_H
#define SCORE_REFINE_ROBUST_H

#include <stdint.h>

#include "score_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct score_refine_robust_settings {
    double  inlier_threshold;  /* c: residual bound of an inlier range, in standard deviations (> 0, finite)       */
    double  rel_threshold;     /* c_rel: the same for a loop closure (> 0, finite)                                  */
    double  mu_step;           /* factor of the GNC parameter between outer iterations (> 1)                        */
    double  min_weight;        /* floor of the weighted precisions, in (0, 1]: every measurement stays a term       */
    int32_t families;          /* bit 0: the ranges, bit 1: the loop closures; 0 is an error                        */
    int32_t max_outer;         /* outer solves (>= 1)                                                               */
    int32_t inner_iters;       /* Levenberg-Marquardt iterations of solves 2, 3, ... (>= 1)                         */
    int32_t max_iters;         /* Levenberg-Marquardt iterations of the first and the last run                      */
    double  tol;               /* gradient tolerance of the first and the last Levenberg-Marquardt run              */
} score_refine_robust_settings;

typedef struct score_refine_robust_info {
    int32_t outer_iterations;  /* solves of the loop (the last run of step 5 is not counted)                        */
    int32_t converged;         /* 1: stopped on binary weights or on a first solve without outliers                 */
    int32_t outliers;          /* ranges with final weight < 1/2                                                    */
    int32_t rel_outliers;      /* loop closures with final weight < 1/2 (0 where that family is off)                */
    double  mu;                /* GNC parameter that produced the final weights (0: the first solve's)              */
    int32_t lm_iterations;     /* Levenberg-Marquardt iterations of all runs                                        */
    int32_t linear_solves;     /* damped normal equations solved                                                    */
    int32_t pcg_iters;         /* PCG iterations they took                                                          */
    double  cost_initial;      /* the unweighted cost at the input point                                            */
    double  cost_final;        /* the cost of the last run, with the final weights                                  */
    double  grad_inf;          /* |J'r|_inf of the last run                                                         */
    double  setup_ms;          /* the handle's create                                                               */
    double  solve_ms;          /* this call                                                                         */
} score_refine_robust_info;

/* inlier_threshold = rel_threshold = 3, mu_step = 1.4, min_weight = 1e-6, tol = 1e-10, families = 1, max_outer = 50,
 * inner_iters = 5, max_iters = 50 */
void score_refine_robust_default_settings(score_refine_robust_settings* rs);

/* poses_in .. landmarks_out: laid out as score_refine_run's.  Further outputs (caller-owned; any may be NULL):
 *   weights, residuals          n_ranges         final weights, r at the final estimate
 *   rel_weights, rel_residuals  loop closures    the same, in the order of the trailing relative-pose entries
 * A family that is off reports weights of 1 and still reports its residuals.
 * Every precision of an enabled family (as given to score_refine_create) must be positive and finite.
 * 0 = ok (info->converged tells how the loop stopped), < 0 = error (score_last_error()). */
int score_refine_robust_run(score_refine* r, const score_refine_robust_settings* rs,
                            const double* poses_in, const double* landmarks_in,
                            double* poses_out, double* landmarks_out,
                            double* weights, double* residuals, double* rel_weights, double* rel_residuals,
                            score_refine_robust_info* info);

/* The residuals above at a given point, with no solve, and for mu > 0 the GNC-TLS weights of step 3 with thresholds c (ranges)
 * and c_rel (loop closures), both > 0 then; mu = 0: weights of 1.  The handle's precisions are not touched.  Any output may be NULL. */
int score_refine_residuals(score_refine* r, const double* poses, const double* landmarks, double mu, double c, double c_rel,
                           double* residuals, double* rel_residuals, double* weights, double* rel_weights);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_REFINE_ROBUST_H */

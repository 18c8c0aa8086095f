/*
 * score_refine_robust_batch.h -- outlier-robust local refinement of MANY graphs in lock-step (HIP library only, like
 * score_refine_batch.h): the GNC-TLS loop of score_refine_robust.h, one per member, on a group handle of score_refine_batch.h.
 *
 * Member g follows the loop score_refine_robust.h states, with its own settings, its own mu, its own count of outer solves and
 * its own place in the schedule (first run, inner runs, last run).  Solve 1 is score_refine_batch_run's.  When a member's run
 * stops: its residuals with the MEASURED precisions, the stop rule, mu, its weights, the next solve's precisions
 * prec * max(w, min_weight); then a new Levenberg-Marquardt run from its current point (lambda back at 1e-6).  Members never
 * wait for one another: a member whose run stopped in one round is solved again in the next, while others are in the middle of
 * a run or have finished for good.  All members whose runs stopped in the same round share one residual launch, one
 * device-to-host read of the per-workgroup partials, one upload of their parameters, one weight launch, one cost evaluation
 * and one gradient.  Members never influence one another: a member's result is what score_refine_robust_run computes on a
 * handle on it alone, up to the rounding of the two conjugate-gradient implementations; a member that stops after solve 1 (no
 * outliers, or every enabled family empty) is score_refine_batch_run's member, bit for bit.
 *
 * The handle keeps the measured precisions in device arrays of its own, made at the first call of this header (that call's
 * solve_ms includes making them): a group handle never used robustly pays no device memory and no launch for them, only the
 * host copies of the range and relative-pose precisions that every group handle keeps after its create.
 */
#ifndef SCORE_REFINE_ROBUST_BATCH_H
#define SCORE_REFINE_ROBUST_BATCH_H

#include <stdint.h>

#include "score_refine_batch.h"
#include "score_refine_robust.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rs: n_settings == 1 (every member shares it) or n_settings == count (member g takes rs[g]); anything else is an error.
 * The settings are checked member by member, as score_refine_robust_run checks them, before anything on the device is
 * touched; the error text names the member.
 * Points as score_refine_batch_run's.
 * weights / residuals: the members' ranges, member after member.
 * rel_weights / rel_residuals: the members' loop closures, member after member.
 * A family a member has not enabled reports weights of 1 and still reports its residuals.
 * Any output may be NULL.  infos: count records or NULL; infos[g] as score_refine_robust_run reports a handle on member g
 * alone (lm_iterations, linear_solves, pcg_iters summed over its runs; cost_final and grad_inf its last run's); setup_ms and
 * solve_ms are the group's.
 *
 * The call always starts from the measured precisions.
 * keep_weights = 0: on every return, an error return included, the handle holds the measured precisions: a later
 *   score_refine_batch_run or score_refine_batch_marginals equals a fresh handle's.
 * keep_weights = 1: on a successful return the precisions the handle's cost reads are prec * w_final in every enabled family of
 *   every member -- the plain weight, not floored by min_weight -- so score_refine_batch_marginals on the same handle gives the
 *   covariances under the final weights (one create serves both).  A plain score_refine_batch_run after keep_weights = 1 also
 *   runs on these weighted precisions, until score_refine_batch_restore or the next score_refine_batch_robust_run.  On an error
 *   return the handle holds the measured precisions.
 * 0 = ok (infos[g].converged tells how member g's loop stopped), < 0 = error (score_last_error()). */
int score_refine_batch_robust_run(score_refine_batch* b, const score_refine_robust_settings* rs, int32_t n_settings,
                                  const double* poses_in, const double* landmarks_in, double* poses_out, double* landmarks_out,
                                  double* weights, double* residuals, double* rel_weights, double* rel_residuals,
                                  int32_t keep_weights, score_refine_robust_info* infos);

/* residuals at given points, with no solve, and for mu[g] > 0 the weights (mu, c, c_rel: count entries each; c[g], c_rel[g] > 0
 * where mu[g] > 0; mu[g] = 0: weights of 1).  The handle's precisions are not touched. */
int score_refine_batch_residuals(score_refine_batch* b, const double* poses, const double* landmarks,
                                 const double* mu, const double* c, const double* c_rel,
                                 double* residuals, double* rel_residuals, double* weights, double* rel_weights);

/* the block kernels read the measured precisions again */
int score_refine_batch_restore(score_refine_batch* b);

/* of the last score_refine_batch_robust_run on the handle: its lock-step rounds, and the passes in which some member's run had
 * stopped and it changed stage (either may be NULL; both 0 before the first run) */
int score_refine_batch_robust_rounds(score_refine_batch* b, int32_t* rounds, int32_t* stage_rounds);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_REFINE_ROBUST_BATCH_H */

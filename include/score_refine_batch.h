/*
 * score_refine_batch.h -- local refinement of MANY graphs in lock-step (HIP library only, like score_marginals.h).
 *
 * score_refine_run takes one graph per handle and meets the host four or five times per Levenberg-Marquardt iteration.  A
 * group handle holds `count` graphs of one dimension as ONE union problem -- the members' unknowns one member after the other,
 * J'J block diagonal on one linear-mode pattern whose chain hint lists every member's chains -- and runs the loop of
 * score_refine_run on every member at once: per round one gather of J'J + lambda_g I, one chain factorisation, one
 * conjugate-gradient solve in which every member has its own alpha, beta, stopping gate
 *   r'M^-1 r <= rel_tol^2 r0'M^-1 r0        (rel_tol = 1e-9, at most 4000 iterations, as score_refine_run)
 * and done word, one trial point and one cost evaluation.  Then every member decides for itself, by the rules of
 * score_refine_run: lambda from 1e-6, x 10 on a rejected step or a failed solve, x 0.1 (floor 1e-12) on acceptance; stop on
 * |J'r|_inf <= tol max(1, cost), on a decrease <= 1e-14 max(1, cost), after 12 rejected attempts, at max_iters.  A member
 * that has stopped costs no further product traffic.  Members never influence one another: a member's result is what a
 * score_refine handle on it alone computes, up to the rounding of the two conjugate-gradient implementations.
 */
#ifndef SCORE_REFINE_BATCH_H
#define SCORE_REFINE_BATCH_H

#include <stdint.h>

#include "score_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct score_refine_batch score_refine_batch;

/* graphs: `count` graphs as score_refine_create takes them, all of one `dim` (a mixed group is an error, score_last_error());
 * every member needs at least one unknown.  The arrays are copied: they may go when the call returns. */
int  score_refine_batch_create(const score_graph* graphs, int32_t count, const score_settings* s, score_refine_batch** out);

/* poses_in / landmarks_in / poses_out / landmarks_out: the members' arrays one after the other, each in score_refine_run's
 * layout (member i's poses follow member i-1's; a member without landmarks takes no room).  Every member keeps its own
 * first pose fixed.  infos: `count` records (or NULL), infos[i] as score_refine_run reports member i; setup_ms and solve_ms
 * are the group's. */
int  score_refine_batch_run(score_refine_batch* b, const double* poses_in, const double* landmarks_in,
                            int32_t max_iters, double tol, double* poses_out, double* landmarks_out,
                            score_refine_info* infos);

void score_refine_batch_destroy(score_refine_batch* b);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_REFINE_BATCH_H */

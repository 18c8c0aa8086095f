/*
 * score_relative_batch.h -- predicted relative poses between listed pairs of poses of EVERY member of a refinement group
 * and their covariances (HIP library only, like score_leverage_batch.h): the Mahalanobis gates of a whole study in one call.
 *
 * score_refine_relative_covariances (include/score_relative.h) works on one graph per handle; on a small world its block
 * solves are latency-bound.  A group handle (score_refine_batch_create, include/score_refine_batch.h) holds the members as
 * ONE union problem whose H = J'J is block diagonal, so one union vector carries one column of every member, all members in
 * one pass over the union matrix.
 *
 * R_ab, t_ab, the error coordinates xi, G and P_c = G_c H_g^-1 G_c' are exactly those of include/score_relative.h, with
 * H_g the member's own H at its point.  Member g with C_g pairs has K_g = DP C_g columns; column j = c DP + q solves
 * H_g x_j = G_c' e_q with the iteration of score_refine_batch_marginals (include/score_marginals_batch.h: its stopping rule
 * and breakdown words per (member, slot)).  Pass k of width W carries column k W + s of every member in slot s, so
 * passes = ceil(max_g K_g / W), a member with K_g <= k W has dropped out of pass k, and a pair may straddle two passes.
 *
 * No atomics and a fixed order everywhere: two calls give the same bits, and a member's outputs are those of a group that
 * holds it alone, bit for bit.
 *
 * Memory: the iteration's vectors and the right-hand sides are those of score_refine_batch_marginals and
 * score_refine_batch_samples (see score_samples_batch.h).  New with the first call and until the handle goes: one int32 per
 * member and, per listed pair, 2 ids, its member and DP^2 + DIM^2 + DIM doubles (the room grows on demand).
 *
 * The call leaves the handle as it found it: a later score_refine_batch_run, _marginals, _samples or _range_variances equals
 * a fresh handle's, bit for bit.
 */
#ifndef SCORE_RELATIVE_BATCH_H
#define SCORE_RELATIVE_BATCH_H

#include <stdint.h>

#include "score_marginals_batch.h"   /* score_marginals_batch_info */
#include "score_relative.h"

#ifdef __cplusplus
extern "C" {
#endif

/* poses / landmarks: the members' points, laid out as score_refine_batch_run's inputs.
 * pair_ptr / pair_a / pair_b: member g lists the pairs pair_a[c] - pair_b[c], c in pair_ptr[g] .. pair_ptr[g + 1], as in
 *   score_refine_batch_range_variances: count + 1 entries, starting at 0, not decreasing; pair_ptr == NULL: nobody lists any.
 *   The ids are member-local POSE ids 0 .. Np_g - 1; the fixed pose 0 is a legitimate end.  Errors, each naming the member
 *   ("member g: ..."): a == b, an id outside 0 .. Np_g - 1 (a landmark has no relative pose).  Pairs listed without their
 *   lists: error.  More pairs in the group than the int32 prefix sums of their columns and blocks hold: error.
 * block_width: 1..16 columns of every member per pass.
 * Outputs, the members' pairs one after the other (pair_ptr's order):
 *   rotations: pairs x DIM x DIM row-major, R_ab.  translations: pairs x DIM, t_ab.
 *   covariances: pairs x DP x DP row-major, column q as computed (not symmetrised).
 *   residuals: pairs x DP, the true residual |G_c'e_q - H_g x_j|_2 from one more product.
 *   iters: pairs x DP, a column's steps, -(steps + 1) where it did not converge.
 * There is no `solutions` output.  Any output may be NULL.
 * info: columns = all columns, passes = ceil(max_g K_g / block_width), pcg_iters per pass the most any (member, slot) took,
 *   summed.  Every member with an empty list: returns 0 with columns = passes = 0 and no device work.
 * Returns 0: all columns converged; 1: some did not (outputs still written); < 0: error (score_last_error()); the handle
 * goes on working after one. */
int score_refine_batch_relative_covariances(score_refine_batch* b, const double* poses, const double* landmarks,
                                            const int32_t* pair_ptr, const int32_t* pair_a, const int32_t* pair_b,
                                            double rel_tol, int32_t max_iters, int32_t block_width,
                                            double* rotations, double* translations, double* covariances,
                                            double* residuals, int32_t* iters,
                                            score_marginals_batch_info* info);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_RELATIVE_BATCH_H */

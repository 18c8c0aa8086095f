/*
 * score_leverage_batch.h -- leverage of the measurements and predicted range variances of EVERY member of a refinement
 * group (HIP library only, like score_samples_batch.h).
 *
 * score_refine_leverage / score_refine_range_variances (include/score_leverage.h) work on one graph per handle; on a small
 * world their block solves are latency-bound.  A group handle (score_refine_batch_create, include/score_refine_batch.h)
 * holds the members as ONE union problem whose H = J'J is block diagonal, so one union vector carries one draw (or one
 * pair's column) of every member, all members in one pass over the union matrix.
 *
 * score_refine_batch_leverage is score_refine_batch_samples (include/score_samples_batch.h) with another use of a solved
 * pass: the draws of member g -- the noise stream keyed by seeds[g] with the member-local measurement number, the probe per
 * member, the stopping rule, the breakdown words, determined, residuals, iters and every field of info -- are those of
 * score_refine_batch_samples with the same seeds, first_sample, n_samples and block_width, bit for bit.  After a pass's
 * verdicts one lane per measurement of every member forms, per converged draw of that member in ascending s,
 * y = J_m delta, t = |y|^2 and v = |z_m - y|^2 (z regenerated, not stored) and adds t, t^2, v, v^2 to running sums: the
 * definitions, the numbering of the measurements and the order of the additions are score_leverage.h's.  A member whose
 * probe fails has all draws unconverged and zero sums; it never touches a neighbour.
 *
 * score_refine_batch_range_variances solves H_g x = g_c for the listed pairs of every member with the iteration of
 * score_refine_batch_marginals (include/score_marginals_batch.h): pass k of width W carries pair k W + c of every member
 * in slot c, with that call's stopping rule and breakdown words per (member, slot).  A member with fewer pairs drops out of
 * the later passes.
 *
 * No atomics and a fixed order everywhere: two calls give the same bits, no sum depends on block_width, and a member's
 * outputs are those of a group that holds it alone, bit for bit.
 *
 * Memory: the iteration's vectors and the draws' buffers are those of score_refine_batch_marginals and
 * score_refine_batch_samples (one allocation for all: see score_samples_batch.h); the right-hand sides g_c use the draws'
 * 16 x 8 bytes per unknown.  New with the first call and until the handle goes: 4 x 8 bytes per measurement of the group
 * (the running sums) and, per listed pair, 2 ids, its member, 2 sums, a variance and a distance (44 bytes; the room grows on
 * demand).  64 worlds of 4 x 1000 poses (448 093 measurements): 14 MB beside the 1 GB of vectors, right-hand sides and block
 * slots.
 *
 * Both calls leave the handle as they found it: a later score_refine_batch_run, _marginals or _samples equals a fresh
 * handle's, bit for bit.
 */
#ifndef SCORE_LEVERAGE_BATCH_H
#define SCORE_LEVERAGE_BATCH_H

#include <stdint.h>

#include "score_samples_batch.h"     /* score_samples_batch_info   */
#include "score_marginals_batch.h"   /* score_marginals_batch_info */

#ifdef __cplusplus
extern "C" {
#endif

/* poses / landmarks, seeds, first_sample, n_samples, block_width, rel_tol, max_iters, residuals, iters, determined, info:
 *   as in score_refine_batch_samples.  A member with S_g = 0 takes no part and no room in the outputs.
 * pair_ptr / pair_a / pair_b: member g lists the hypothetical ranges pair_a[c] - pair_b[c], c in
 *   pair_ptr[g] .. pair_ptr[g + 1]; the ids are member-local variable ids as in score_refine_leverage (poses 0 .. Np_g - 1,
 *   then the landmarks; the fixed pose 0 is a legitimate end).  pair_ptr has count + 1 entries, starts at 0 and does not
 *   decrease; pair_ptr == NULL: no pairs for anyone.  Errors: a == b, an id out of the member's range, pairs listed for a
 *   member with S_g = 0.
 * Outputs:
 *   lev_sum, lev_sq, red_sum, red_sq: member after member (members with S_g > 0), M_g = n_rel + n_rng + n_pri entries each,
 *     numbered and defined as in score_leverage.h: the SUMS of t, t^2, v, v^2 over the member's converged draws;
 *   pair_sum, pair_sq: the members' pairs one after the other (pair_ptr's order): the sums of (g_c'delta)^2 and its square;
 *   residuals / iters / determined / info: those of score_refine_batch_samples.
 * Any output may be NULL.
 * Returns 0: all draws converged; 1: some did not (outputs still written, the sums over the converged draws); < 0: error
 * (score_last_error()); the handle goes on working after one. */
int score_refine_batch_leverage(score_refine_batch* b, const double* poses, const double* landmarks,
                                const uint64_t* seeds, int64_t first_sample, const int32_t* n_samples,
                                const int32_t* pair_ptr, const int32_t* pair_a, const int32_t* pair_b,
                                double rel_tol, int32_t max_iters, int32_t block_width,
                                double* lev_sum, double* lev_sq, double* red_sum, double* red_sq,
                                double* pair_sum, double* pair_sq,
                                double* residuals, int32_t* iters, int32_t* determined,
                                score_samples_batch_info* info);

/* pair_ptr / pair_a / pair_b: as above; every member takes part, a member may list none (pair_ptr == NULL: nobody lists any).
 * block_width: 1..16 pairs of every member per pass.
 * Outputs, the members' pairs one after the other:
 *   variances: g_c'x_c; distances: |p_a - p_b| at the point; residuals: |g_c - H_g x_c|_2 from one more product;
 *   iters: a column's steps, -(steps + 1) where it did not converge.
 * info: columns = all pairs, passes = ceil(max_g C_g / block_width), pcg_iters per pass the most any (member, slot) took,
 *   summed.  Every member with an empty list: returns 0 with columns = passes = 0 and no device work.
 * There is no `solutions` output.  Any output may be NULL.
 * Returns 0: all columns converged; 1: some did not (outputs still written); < 0: error (score_last_error()); the handle
 * goes on working after one. */
int score_refine_batch_range_variances(score_refine_batch* b, const double* poses, const double* landmarks,
                                       const int32_t* pair_ptr, const int32_t* pair_a, const int32_t* pair_b,
                                       double rel_tol, int32_t max_iters, int32_t block_width,
                                       double* variances, double* distances, double* residuals, int32_t* iters,
                                       score_marginals_batch_info* info);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_LEVERAGE_BATCH_H */

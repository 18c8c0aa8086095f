/*
 * score_select_batch.h -- greedy selection of candidate ranges by joint information gain for EVERY member of a refinement
 * group (HIP library only, like score_leverage_batch.h).
 *
 * score_refine_select_ranges (include/score_select.h) answers "k more ranges out of these C candidates -- which k?" on one
 * graph per handle: ceil(C / 16) latency-bound block solves and one pivoted Cholesky factorisation in a single workgroup.  A
 * study asks it of every world.  On a group handle (score_refine_batch_create, include/score_refine_batch.h) the columns
 * x_c = H_g^-1 g_c are those of score_refine_batch_range_variances (include/score_leverage_batch.h): pass k of width W
 * carries candidate k W + s of every member in slot s.  After each pass one lane per listed pair of the whole group writes
 * the cross terms P_g[c C_g + k W + s] = g_c'x_{g,s} of its member; after the last pass one launch forms
 * A_g = I + D_g (P_g + P_g')/2 D_g for every member and one launch runs the members' factorisations side by side, one
 * workgroup each.
 *
 * Contracts:
 *  1. variances, distances, residuals, iters and info.solve are those of score_refine_batch_range_variances on the same
 *     pairs, points, rel_tol, max_iters and block_width, bit for bit; a later call of that function, of
 *     score_refine_batch_run, _marginals or _samples equals a fresh handle's.
 *  2. The diagonal of a member's P is its `variances`, bit for bit; column d of P is "as computed", as in score_select.h.
 *  3. A member's selection is the rule of score_select.h (csrc/score_select_rule.hpp) on its own matrix with its own
 *     exclusions: order, gains, pick_variances and remaining equal score_select_greedy on that member's returned matrix,
 *     precisions and exclusions, bit for bit.
 *  4. A member's outputs are those of a group that holds it alone, bit for bit; they do not depend on block_width, and two
 *     calls give the same bits.
 *  5. fp64 throughout, no atomics, fixed-order sums.
 *
 * Memory: beside the buffers of score_refine_batch_range_variances, new with the first call, grown on demand and kept until
 * the handle goes (device allocations of their own, not the handle's arena): 8 C_g^2 bytes of P and 8 C_g k_g bytes of L per
 * member, and per listed pair a precision, an exclusion word and a remaining variance.  64 worlds with C = 256 and k = 32:
 * 33.6 MB of P, 4.2 MB of L.
 */
#ifndef SCORE_SELECT_BATCH_H
#define SCORE_SELECT_BATCH_H

#include <stdint.h>

#include "score_leverage_batch.h"
#include "score_marginals_batch.h"
#include "score_select.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct score_select_batch_info {
    score_marginals_batch_info solve;   /* the group's block PCG, as score_refine_batch_range_variances reports it */
    int32_t members, candidates, picked, excluded;   /* members of the group; listed pairs, picks and exclusions of all */
    double  total_gain;                 /* the members' total gains added in member order, nats */
    double  asymmetry;                  /* the largest max |P_cd - P_dc| of any member */
    double  cross_ms, greedy_ms;
} score_select_batch_info;

/* pair_ptr / pair_a / pair_b: as in score_refine_batch_range_variances: member g lists the candidates pair_a[c] - pair_b[c],
 *   c in pair_ptr[g] .. pair_ptr[g + 1], by member-local variable ids (duplicate pairs are allowed); pair_ptr has count + 1
 *   entries; a member may list none.
 * precisions: one per listed pair, finite and positive.
 * k: one per member.  With C_g > 0 candidates 1 <= k[g] <= min(C_g, 256) and C_g <= 4096; with C_g == 0, k[g] must be 0.
 * min_gain >= 0: for all members.
 * The sum over the members of C_g^2 may not exceed 2^28 entries (2 GiB of P): an error that names the figure.
 * Outputs:
 *   order, gains, pick_variances: member after member, k[g] entries each: the picks in their order, padded with -1 / 0 / 0;
 *   picked, total_gains: one entry per member (total_gains[g]: the member's gains added in the order of its picks);
 *   variances, distances, remaining, residuals, iters: the members' pairs one after the other (pair_ptr's order), as in
 *     score_select.h and score_leverage_batch.h;
 *   matrix: normally NULL; else the members' C_g x C_g blocks one after the other, each P as computed.
 * A column that did not converge excludes its candidate in its member.  Any output may be NULL.
 * Every member with an empty list: returns 0 with zeros in picked, total_gains and info, and no device work.
 * Returns 0; 1: some column did not converge (outputs still written); < 0: error (score_last_error()); the handle goes on
 * working after one. */
int score_refine_batch_select_ranges(score_refine_batch* b, const double* poses, const double* landmarks,
                                     const int32_t* pair_ptr, const int32_t* pair_a, const int32_t* pair_b,
                                     const double* precisions, const int32_t* k, double min_gain,
                                     double rel_tol, int32_t max_iters, int32_t block_width,
                                     int32_t* order, double* gains, double* pick_variances,
                                     int32_t* picked, double* total_gains,
                                     double* variances, double* distances, double* remaining,
                                     double* residuals, int32_t* iters, double* matrix,
                                     score_select_batch_info* info);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_SELECT_BATCH_H */

/*
 * score_samples_batch.h -- draws from the Gaussian posterior of EVERY member of a refinement group (HIP library only, like
 * score_marginals_batch.h).
 *
 * score_refine_samples (include/score_samples.h) draws on one graph per handle; on a small world its block solve is
 * latency-bound.  A group handle (score_refine_batch_create, include/score_refine_batch.h) holds the members as ONE union
 * problem whose H = J'J is block diagonal, so one union vector carries one draw of every member: pass k of width W solves
 * draw first_sample + k W + c of every member in slot c, all members in one pass over the union matrix.  A member with
 * fewer draws drops out of the later passes; the slots of a pass are the smallest of 1, 2, 4, 8, 16 that hold the most
 * live slots of any member.
 *
 * Per member the contract is that of score_samples.h: z ~ N(0, I), b = J'z, H delta = b, the stopping rule
 * r'M^-1 r <= rel_tol^2 r0'M^-1 r0 and the breakdown words of score_refine_batch_marginals, per (member, slot).  The noise of
 * member g is the stream of score_samples.h keyed by seeds[g] with the member-local measurement number m: what a single
 * handle on that graph draws with seed = seeds[g].
 *
 * The probe of score_samples.h runs per member and decides per member: before the passes ONE slot of the group's iteration
 * solves H_g x = xi_g for every member with draws (xi_g[i]: Philox purpose 14 keyed by seeds[g], counter = the member-local
 * unknown i; budget 4000 iterations).  Member g is determined where that column converged and its true residual satisfies
 * |xi_g - H_g x|_2 <= sqrt(rel_tol) |xi_g|_2; otherwise ALL draws of that member are reported as not converged and left out
 * of its sums.  A singular member never affects another.
 *
 * Members never influence one another: a member's outputs are those of a group that holds it alone, bit for bit.
 *
 * Memory: the iteration's vectors are those of score_refine_batch_marginals (one allocation for both: 6 buffers x NV x 8
 * bytes per unknown of the group, NV the slots in use).  The draws add, with the first call and until the handle goes:
 * 16 x 8 bytes per unknown (the right-hand sides), 16 x 8 bytes per block slot of J'z (in 2-D | 3-D: 6 | 12 per relative
 * pose, 4 | 6 per range, 2 | 3 per prior), the running sums (dp + 1 doubles per pose unknown, d + 1 per landmark unknown;
 * dp = 3 | 6) and, where noise is asked for, 16 x 8 bytes per residual row.  64 worlds of 4 x 1000 poses (768 576 unknowns,
 * about 2.3 M block slots): 0.1 GB of right-hand sides and 0.3 GB of block slots beside the 0.6 GB of vectors.
 *
 * The call leaves the handle as it found it: a later score_refine_batch_run or score_refine_batch_marginals equals a fresh
 * handle's, bit for bit.
 */
#ifndef SCORE_SAMPLES_BATCH_H
#define SCORE_SAMPLES_BATCH_H

#include <stdint.h>

#include "score_refine_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct score_samples_batch_info {
    int32_t members;       /* members of the group                                                                  */
    int32_t samples;       /* draws asked for, all members                                                          */
    int32_t passes;        /* passes over the union matrix (the probe's is not counted)                             */
    int32_t pcg_iters;     /* per pass the most any (member, slot) took, summed; the probe is excluded              */
    int32_t unconverged;   /* draws that hit max_iters or broke down, and every draw of a member whose probe failed */
    int32_t singular;      /* members whose probe failed                                                            */
    double  max_residual;  /* largest |b_s - H_g delta_s|_2 of the call                                             */
    double  setup_ms;      /* blocks at the points, H, chain factors, buffers, the probe column                     */
    double  rhs_ms;        /* noise, J'z and its gather, all passes                                                 */
    double  solve_ms;      /* the solves, residuals, moments and the copies back                                    */
} score_samples_batch_info;

/* poses / landmarks: the members' points one after the other, laid out as score_refine_batch_run's inputs.
 * seeds: count entries, one noise stream per member.
 * first_sample (shared) >= 0; n_samples: count entries S_g >= 0, at least one > 0; first_sample + max S_g <= 2^32.  A member
 *   with S_g = 0 takes no part: no probe, no draws, no room in the outputs, no product traffic.
 * var_ptr / vars: as in score_refine_batch_marginals -- member g selects the member-local variables
 *   vars[var_ptr[g] .. var_ptr[g + 1]) (pose 0 of a member is fixed: error; duplicates: error; var_ptr starts at 0 and
 *   does not decrease).  A member may list none: it has no steps, its draws, moments and means are still formed.
 *   C_g = the scalar unknowns of its variables.
 * block_width: 1..16 draws of every member per pass.
 * Outputs, member after member (members with S_g > 0), each in the layout of score_samples.h:
 *   moments: the packed per-variable sums over the member's converged draws; means: n_g;
 *   steps: S_g x C_g; rhs: S_g x n_g; noise: S_g x rows_g;
 *   residuals / iters: sum of S_g entries, a draw's steps as -(steps + 1) where it did not converge.
 * determined: count entries -- 1 the member's probe passed, 0 it failed, -1 S_g = 0.
 * Any output may be NULL.
 * Returns 0: all draws converged; 1: some did not (outputs still written); < 0: error (score_last_error()); the handle
 * goes on working after one. */
int score_refine_batch_samples(score_refine_batch* b, const double* poses, const double* landmarks,
                               const uint64_t* seeds, int64_t first_sample, const int32_t* n_samples,
                               const int32_t* var_ptr, const int32_t* vars,
                               double rel_tol, int32_t max_iters, int32_t block_width,
                               double* moments, double* means, double* steps, double* rhs, double* noise,
                               double* residuals, int32_t* iters, int32_t* determined,
                               score_samples_batch_info* info);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_SAMPLES_BATCH_H */

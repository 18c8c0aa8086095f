/*
 * score_spectrum_batch.h -- the weakest modes of EVERY member of a refinement group (HIP library only, like
 * score_marginals_batch.h).
 *
 * score_refine_spectrum (include/score_spectrum.h) gives the lowest eigenpairs of H = J'J of one graph per handle, and reads
 * a 48 x 48 pencil back to the host in every iteration.  A group handle (score_refine_batch_create,
 * include/score_refine_batch.h) holds the members as ONE union problem whose H is block diagonal, so one union vector
 * carries one vector of every member: six blocks of 16 union vectors run LOBPCG with a block of 16 on every member at once,
 * in lock-step rounds.  The Rayleigh-Ritz step runs on the device, one workgroup per member; per round the host reads and
 * writes a few words per member (16 residual norms, a status, a mode), never a pencil.
 *
 * Per member g the contract is that of score_spectrum.h: A_g = H_g + sigma_g I with sigma_g = shift_rel * h_max_g
 * (h_max_g = max diag H_g), a pair counts as converged at |A_g x - theta x|_2 <= rel_tol * h_max_g, done columns are soft
 * locked, and a member ends only on the residuals of a true product A_g X.  Members never influence one another: a member's
 * outputs are those of a group that holds it alone, bit for bit.
 *
 * Memory: the blocks are device allocations of the handle's own (not its arena's); they come with the first call and go
 * with the handle: 8 buffers x 16 vectors x 8 bytes per unknown of the group -- 64 worlds of 12 000 unknowns take about
 * 0.8 GB.
 *
 * The call leaves the handle as it found it: a later score_refine_batch_run equals a fresh handle's run bit for bit.
 */
#ifndef SCORE_SPECTRUM_BATCH_H
#define SCORE_SPECTRUM_BATCH_H

#include <stdint.h>

#include "score_refine_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct score_spectrum_batch_info {
    int32_t members;       /* members of the group                                                                 */
    int32_t modes;         /* k asked of every member                                                              */
    int32_t block;         /* vectors iterated per member (16)                                                     */
    int32_t rounds;        /* lock-step passes queued                                                              */
    int32_t unconverged;   /* members with a pair above tolerance (or broken down)                                 */
    double  max_residual;  /* largest |H_g v - lambda v|_2 of the call                                             */
    double  setup_ms;      /* blocks at the points, H, max diag H, chain factors, buffers                          */
    double  solve_ms;      /* the rounds and the copy back                                                         */
} score_spectrum_batch_info;

/* poses / landmarks: the members' points one after the other, laid out as score_refine_batch_run's inputs.  The unknowns
 * of a member and their order are score_refine_marginals' (pose 0 of the member fixed).
 * k: 1..16 pairs of every member.  A member with fewer than 48 unknowns: error naming the member.
 * values: count x k, ascending per member.
 * vectors: member g: k x n_g row-major, unit 2-norm; the members one after the other.
 * residuals: count x k, |H_g v - lambda v|_2 from one more product.
 * iterations: count, the LOBPCG iterations of the member -- as -(it + 1) where not all k pairs converged or the member
 *   broke down.
 * h_max: count, max diag H_g.  Any output may be NULL.
 * Returns 0: every member has all k pairs at rel_tol * h_max_g; 1: some has not (outputs still written); < 0: error
 * (score_last_error()); the handle goes on working after one. */
int score_refine_batch_spectrum(score_refine_batch* b, const double* poses, const double* landmarks,
                                int32_t k, double rel_tol, int32_t max_iters, double shift_rel,
                                double* values, double* vectors, double* residuals, int32_t* iterations,
                                double* h_max, score_spectrum_batch_info* info);

/* The device Rayleigh-Ritz step alone, on the caller's pencils (no handle; device 0): count pairs (GA, GB) = (S'AS, S'S)
 * of 48 x 48 row-major doubles, S = [X | W | P] with 16 columns each.  Per pencil the 16 lowest Ritz values theta
 * (count x 16), the coefficients coef (count x 48 x 16 row-major, c'(GB)c = 1 per column), status (0: ok; 1: the P block
 * was left out; 2: breakdown -- theta and coef of that pencil are not written) and kept (directions left after the
 * deflation of the scaled Gram matrix).  The steps and thresholds are those of the single solver's host routine. */
int score_spectrum_ritz(int32_t count, const double* GA, const double* GB, double* theta, double* coef,
                        int32_t* status, int32_t* kept);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_SPECTRUM_BATCH_H */

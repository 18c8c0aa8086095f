/*
 * score_marginals_batch.h -- marginal covariances of EVERY member of a refinement group (HIP library only, like
 * score_marginals.h).
 *
 * score_refine_marginals solves H X = E_S for one graph per handle; a Monte-Carlo study wants the covariances of dozens of
 * small worlds, and on a small world every launch of that solve is latency-bound.  A group handle (score_refine_batch_create,
 * include/score_refine_batch.h) already holds the members as ONE union problem whose H = J'J is block diagonal, so one union
 * vector carries one unit column of every member at once: a block of up to 16 union vectors advances 16 columns of all
 * members through the chain-preconditioned conjugate-gradient iteration of score_marginals.h in one pass over the union
 * matrix per iteration.  Every (member, slot) pair has its own alpha, beta, stopping gate
 *   r'M^-1 r <= rel_tol^2 r0'M^-1 r0
 * and done word; a column reports its true residual |e_c - H x_c|_2, computed with one more product after its pass.
 * Members never influence one another.
 *
 * Pass k of width W solves column k W + c of every member in slot c; a member with fewer columns drops out of the later
 * passes and costs no product traffic there.
 *
 * Memory: the block's vectors are device allocations of the handle's own (not its arena's); they come with the first call,
 * grow when a later call needs more slots, and go with the handle: 6 buffers x slots x 8 bytes per unknown of the group --
 * 64 worlds of 12 000 unknowns at 16 slots take about 0.6 GB.
 *
 * The call leaves the handle as it found it: a later score_refine_batch_run equals a fresh handle's run bit for bit.
 */
#ifndef SCORE_MARGINALS_BATCH_H
#define SCORE_MARGINALS_BATCH_H

#include <stdint.h>

#include "score_refine_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct score_marginals_batch_info {
    int32_t columns;       /* sum of C_g: scalar unknowns of the selected variables of all members                 */
    int32_t passes;        /* ceil(max_g C_g / block_width)                                                       */
    int32_t pcg_iters;     /* iterations queued: per pass the most any (member, slot) took, summed                */
    int32_t unconverged;   /* columns that hit max_iters or broke down (non-finite r'z or p'w, p'w <= 0)          */
    double  max_residual;  /* largest |e_c - H x_c|_2                                                             */
    double  setup_ms;      /* blocks at the points, H, chain factors, buffers                                     */
    double  solve_ms;      /* the passes, residuals and the copy back                                             */
} score_marginals_batch_info;

/* poses / landmarks: the members' points one after the other, laid out as score_refine_batch_run's inputs.
 * var_ptr: count + 1 positions into vars; member g lists vars[var_ptr[g] .. var_ptr[g + 1]).  A member may list none: it
 *   takes no room in the outputs.
 * vars: member-local variable ids as in score_refine_marginals (0..Np_g-1 poses, then the member's landmarks); pose 0 of a
 *   member is fixed: error.  Duplicates within a member: error.  Columns per variable in the order of score_marginals.h;
 *   C_g: the columns of member g.
 * block_width: 1..16 columns of every member per pass.
 * joint: the members' C_g x C_g row-major matrices one after the other, column c as computed (not symmetrised).
 * residuals, iters: sum of C_g entries in the same order; iters holds the steps a column took -- as -(steps + 1) where it
 *   did not converge.  Any output may be NULL.
 * Returns 0: all columns converged; 1: some did not (outputs still written); < 0: error (score_last_error()). */
int score_refine_batch_marginals(score_refine_batch* b, const double* poses, const double* landmarks,
                                 const int32_t* var_ptr, const int32_t* vars,
                                 double rel_tol, int32_t max_iters, int32_t block_width,
                                 double* joint, double* residuals, int32_t* iters,
                                 score_marginals_batch_info* info);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_MARGINALS_BATCH_H */

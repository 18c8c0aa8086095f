/*
 * score_samples.h -- draws from the Gaussian posterior of a refined estimate (HIP library only, like score_marginals.h).
 *
 * At a point (poses, landmarks) of a refinement handle (score_refine_create, include/score_hip.h) the cost is |r(x)|^2 with
 * the whitened residual r and its Jacobian J; H = J'J is the information matrix in the refinement's own unknowns.  A draw
 * of N(0, H^-1) needs no factor of H:
 *
 *     z ~ N(0, I_m),   b = J'z,   H delta = b   =>   Cov(delta) = H^-1 J'J H^-1 = H^-1.
 *
 * The call forms z and b for up to 16 draws in one pass over the measurements, solves the block with the
 * chain-preconditioned lock-step conjugate-gradient iteration of score_refine_marginals (same kernels, same stopping
 * rule r'M^-1 r <= rel_tol^2 r0'M^-1 r0, same breakdown words) and reduces the draws to per-variable sums on the device.
 *
 * A singular H (a variable the measurements do not determine) does not stop these solves -- J'z lies in the range of J'J --
 * so every call first solves H x = xi for one random vector xi (Philox purpose 14, the same iteration, rel_tol, a budget of
 * 4000 iterations): where that column does not converge, or its true residual |xi - H x|_2 exceeds sqrt(rel_tol) |xi|_2,
 * H is singular or nearly so and EVERY draw of the call is reported as not converged.
 *
 * The noise is counter based: component q of measurement m in draw s is
 *     component (q & 1) of the Box-Muller pair of Philox4x32-10(key = seed, counter = (13, m, s, q >> 1))
 * with s the GLOBAL draw index first_sample + k, so a draw does not depend on n_samples, on block_width or on the other
 * draws of the call.  Measurements m: the relative poses in score_graph's order, then the ranges, then the landmark
 * priors.  Rows q of a measurement: relative pose -- the d translation rows, then the d x d rows of R_j - R_i R~,
 * row-major (6 | 12); range -- one; prior -- d.
 */
#ifndef SCORE_SAMPLES_H
#define SCORE_SAMPLES_H

#include <stdint.h>

#include "score_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct score_samples_info {
    int32_t samples;       /* draws asked for                                                                       */
    int32_t batches;       /* blocks of draws solved                                                                */
    int32_t pcg_iters;     /* per block the most any of its draws took, summed                                      */
    int32_t unconverged;   /* draws that hit max_iters or broke down, all draws where the probe failed: left out of moments / means */
    double  max_residual;  /* largest |b_s - H delta_s|_2                                                           */
    double  setup_ms;      /* blocks at the point, H, chain factors, buffers, the probe column                      */
    double  rhs_ms;        /* noise, J'z and its gather, all blocks                                                 */
    double  solve_ms;      /* the solves, residuals, moments and the copies back                                    */
} score_samples_info;

/* poses / landmarks: the point, laid out as score_refine_run's inputs.
 * vars / n_vars: the variables whose steps are wanted, identified and ordered as in score_refine_marginals (pose 0 is
 *   fixed: error; duplicates: error); NULL / 0: no steps.  C = their scalar unknowns.
 * n_samples >= 1, first_sample >= 0 and first_sample + n_samples <= 2^32 (the draw index is a 32-bit counter); block_width: 1..16 draws per block (the unsplit chain kernel is required, chain_split = 0).
 * moments: per variable with unknowns -- poses 1..Np-1 (dp x dp each, row-major; dp = 3 | 6), then the landmarks (d x d
 *   each) -- the SUM over the converged draws, ascending s, of delta_v delta_v' (not divided by their number).
 * means: n, the sums of delta.
 * steps: n_samples x C.  rhs: n_samples x n, b_s.  noise: n_samples x rows, z in (m, q) order.
 * residuals: n_samples, |b_s - H delta_s|_2.  iters: n_samples, the steps a draw took -- as -(steps + 1) where it did not
 *   converge.  Any output may be NULL.
 * Returns 0: all draws converged; 1: some did not (outputs still written); < 0: error (score_last_error()). */
int score_refine_samples(score_refine* r, const double* poses, const double* landmarks,
                         uint64_t seed, int64_t first_sample, int32_t n_samples,
                         const int32_t* vars, int32_t n_vars,
                         double rel_tol, int32_t max_iters, int32_t block_width,
                         double* moments, double* means, double* steps, double* rhs, double* noise,
                         double* residuals, int32_t* iters,
                         score_samples_info* info);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_SAMPLES_H */

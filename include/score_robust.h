/*
 * score_robust.h -- outlier-robust range measurements for the SCORE relaxation: graduated non-convexity with a
 * truncated-least-squares loss (GNC-TLS; Yang, Antonante, Tzoumas, Carlone, RA-L 2020) over the range measurements of
 * factor graphs (struct score_graph, include/score_hip.h).  Odometry, loop closures and landmark priors keep weight 1.
 *
 * The loop, per graph (weights w = 1, c = inlier_threshold):
 *   1. solve the SOCP relaxation with range precisions prec_k * max(w_k, min_weight);
 *   2. r_k = sqrt(prec_k) * max(0, |t_a - t_b| - dist_k) from the relaxation's translations (the square root of the range's
 *      own term in the relaxed objective);
 *   3. stop if this was the first solve and 2 max r^2 <= c^2 (no outliers: the result is the plain solve), if a later solve
 *      ran on weights that are all within 1e-6 of 0 or 1 (converged), or after max_outer solves (not converged);
 *   4. mu = c^2 / (2 max r^2 - c^2) after the first solve, mu <- mu_step * mu after every later one, and
 *        w = 1 if r^2 <= mu / (mu + 1) c^2,   w = 0 if r^2 >= (mu + 1) / mu c^2,   w = c / r sqrt(mu (mu + 1)) - mu otherwise.
 * The estimate, the weights and the residuals a graph reports are those of its last solve.
 *
 * The graphs' measurement arrays go to the device once; every outer solve builds its handle from them there
 * (score_create_from_graphs' device assembler), the weights are computed by kernels from the solution on the device, and one
 * device-to-host read per outer iteration brings back the per-graph control records and the next weights.  A batch of
 * graphs advances in lock-step; a graph that stops leaves the next handle.
 */
#ifndef SCORE_ROBUST_H
#define SCORE_ROBUST_H

#include <stdint.h>

#include "score_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct score_robust_settings {
    double  inlier_threshold;  /* c: residual bound of an inlier, in standard deviations (> 0)          */
    double  mu_step;           /* factor of the GNC parameter between outer iterations (> 1)              */
    double  min_weight;        /* floor of the weighted precisions, in (0, 1]: every range stays a term   */
    int32_t max_outer;         /* outer solves per graph (>= 1)                                          */
    int32_t qcqp_directions;   /* ranges output: 0 = SOCP distances (n_ranges x 1), 1 = QCQP directions (x d) */
} score_robust_settings;

typedef struct score_robust_info {
    int32_t outer_iterations;  /* solves of this graph                                                   */
    int32_t converged;         /* 1: stopped on binary weights or on a first solve without outliers        */
    int32_t outliers;          /* ranges with final weight < 1/2                                          */
    int32_t reserved;
    double  mu;                /* GNC parameter that produced the final weights (0: the first solve's)     */
    double  setup_ms;          /* handle setup of all outer solves (the handles this graph was part of)    */
    double  solve_ms;          /* solves of all outer iterations                                          */
    double  total_ms;          /* wall time from the call's start to this graph's stop                    */
} score_robust_info;

void score_robust_default_settings(score_robust_settings* rs);

/* `count` graphs of one dimension (their `relaxation` field: 0 = SOCP, 1 = QCQP answered through the SOCP, as
 * qcqp_directions = 1).  Outputs (caller-owned, concatenated graph after graph; any may be NULL):
 *   weights, residuals  n_ranges          final weights and the last solve's r
 *   poses .. degenerate                   as score_read_estimates writes them for a handle of all graphs
 *   infos, rinfos       count             the last solve's score_info, the loop's record
 * Every range precision must be positive and finite.  0 = ok, < 0 = error (score_last_error()). */
int score_robust_solve(const score_graph* graphs, int32_t count, const score_settings* s, const score_robust_settings* rs,
                       double* weights, double* residuals, double* poses, double* relaxed, double* landmarks, double* ranges,
                       int32_t* degenerate, score_info* infos, score_robust_info* rinfos);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_ROBUST_H */

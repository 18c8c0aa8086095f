/*
 * score_robust.h -- outlier-robust range measurements and loop closures for the SCORE relaxation: graduated non-convexity
 * with a truncated-least-squares loss (GNC-TLS; Yang, Antonante, Tzoumas, Carlone, RA-L 2020) over the range measurements
 * and / or the loop closures of factor graphs (struct score_graph, include/score_hip.h).  Odometry and landmark priors keep
 * weight 1.
 *
 * The loop over the ranges alone (score_robust_solve), per graph (weights w = 1, c = inlier_threshold):
 *   1. solve the SOCP relaxation with range precisions prec_k * max(w_k, min_weight);
 *   2. r_k = sqrt(prec_k) * max(0, |t_a - t_b| - dist_k) from the relaxation's translations (the square root of the range's
 *      own term in the relaxed objective);
 *   3. stop if this was the first solve and 2 max r^2 <= c^2 (no outliers: the result is the plain solve), if a later solve
 *      ran on weights that are all within 1e-6 of 0 or 1 (converged), or after max_outer solves (not converged);
 *   4. mu = c^2 / (2 max r^2 - c^2) after the first solve, mu <- mu_step * mu after every later one, and
 *        w = 1 if r^2 <= mu / (mu + 1) c^2,   w = 0 if r^2 >= (mu + 1) / mu c^2,   w = c / r sqrt(mu (mu + 1)) - mu otherwise.
 * The estimate, the weights and the residuals a graph reports are those of its last solve.
 *
 * The loop closures are the second family (score_robust_solve_rel, bit 1 of `families`; threshold c_rel = rel_threshold).  A
 * loop closure e = (i -> j) is one of the trailing n_rel - sum(chain_len - 1) relative-pose entries of its graph, measured
 * kappa, tau, t~, R~.  With the relaxed blocks X_v = [R_v | t_v] of the solve (the pinned pose is [I | 0]),
 *   r_e = sqrt( kappa sum_k (t_j[k] - t_i[k] - sum_c R_i[k,c] t~[c])^2  +  tau sum_{k,c} (R_j[k,c] - sum_m R_i[k,m] R~[m,c])^2 )
 * -- the square root of the term's own value in the relaxed objective, with the measured precisions (never the weighted ones),
 * evaluated in this order without fused multiply-add.  With the families f that are enabled (ranges: c_f = c, loop
 * closures: c_f = c_rel) a graph keeps ONE mu for all of them:
 *   first solve: if no enabled family has 2 max r_f^2 > c_f^2, stop converged (the result is the plain solve); otherwise
 *                mu = min over the families with 2 max r_f^2 > c_f^2 of c_f^2 / (2 max r_f^2 - c_f^2) (the most convex start);
 *   later solves: mu <- mu_step * mu;
 *   weights: w = the rule of step 4 with (r, mu, c_f); the next precisions of a loop closure are kappa * max(w, min_weight) and
 *            tau * max(w, min_weight);
 *   stop: a later solve ran on weights that are binary (within 1e-6) in every enabled family, or after max_outer solves.
 * With the range family alone every operation is the one of the loop above.
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
    int32_t rel_outliers;      /* loop closures with final weight < 1/2 (0 where that family is off)      */
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

/* The same loop over the families of `families` (bit 0: the ranges, bit 1: the loop closures; 0 is an error);
 * score_robust_solve is this call with families = 1.  rel_threshold: c_rel > 0, read only when bit 1 is set.  Further outputs
 * (written when bit 1 is set; may be NULL):
 *   rel_weights, rel_residuals   loop closures, graph after graph (in the order of each graph's trailing relative-pose entries)
 * With bit 0 clear the ranges keep weight 1 (`weights` all 1) and `residuals` are still those of the last solve.  With bit 1 set
 * every loop closure's kappa and tau must be positive and finite. */
int score_robust_solve_rel(const score_graph* graphs, int32_t count, const score_settings* s, const score_robust_settings* rs,
                           int32_t families, double rel_threshold, double* weights, double* residuals, double* rel_weights,
                           double* rel_residuals, double* poses, double* relaxed, double* landmarks, double* ranges,
                           int32_t* degenerate, score_info* infos, score_robust_info* rinfos);

#ifdef __cplusplus
}
#endif
#endif /* SCORE_ROBUST_H */

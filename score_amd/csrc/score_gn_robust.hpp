// score_gn_robust.hpp -- outlier-robust refinement (include/score_refine_robust.h states the loop in full): GNC-TLS re-weighting
// of the ranges and / or the loop closures on the residuals of the maximum-likelihood cost, around the Levenberg-Marquardt loop
// of score_gn.hpp on one refinement handle.
//
// Device: two streaming kernels, one measurement of the asked families per lane (ranges first, then the loop closures -- the
// trailing relative-pose entries):
//   k_gn_robust_resid   r = gn_range_resid / gn_rel_resid (score_gn.hpp: the square root of the block functions' own cost) at the
//                       point, with the MEASURED precisions the handle keeps beside the arrays the block kernels read; per block
//                       and family: max r^2 (non-finite r: +inf) and how many weights of this solve are more than 1e-6 from 0 and
//                       from 1.  block_max / block_sum only: the host folds the partials in block order, as eval_at does.
//   k_gn_robust_weight  w = gnc_tls_weight(r, mu, c_f) (score_robust.hpp, as it stands; mu is an argument, mu = 0: w = 1) and,
//                       with `apply`, the next solve's precisions prec * max(w, min_weight) into the very arrays k_gn_blocks /
//                       k_gn_blocks3 read (rng_prec, rel_kappa, rel_tau): the block kernels stay as they are.
// Host: gn_robust_refine, a template over the backend concept of gn_levenberg_marquardt plus three hooks; the stop rule is the
// pure function robust_decide of score_robust.hpp, the relaxation's.  One device-to-host read per outer iteration (the
// partials) beyond what the LM loop reads.
#pragma once

#include "../../include/score_refine_robust.h"
#include "score_gn_kernels.hpp"
#include "score_robust.hpp"

namespace score {

constexpr int kGnRobustRanges = 1, kGnRobustClosures = 2;   // the bits of `families`
constexpr int kGnRobustPart = 4;   // doubles per block in the partials: max r^2 (ranges, closures), non-binary weights (ranges, closures)

struct GnRobustDev {
    GnDev g;                  // the graph as the block kernels see it
    int dim;
    int64_t n_a, n_b;         // lanes: ranges [0, n_a), loop closures [n_a, n_a + n_b)  (a family that is not asked for: 0)
    int64_t first_lc;         // loop closure e is relative-pose entry first_lc + e
    const double *prec0, *kappa0, *tau0;   // the measured precisions (kappa0, tau0: loop-closure order)
    double *prec, *kappa, *tau;            // what the block kernels read: rng_prec, rel_kappa, rel_tau
    double *r_rng, *r_lc, *w_rng, *w_lc;   // residuals, weights
};

__device__ __forceinline__ double gn_robust_nonbinary(double w) { return (fabs(w) <= 1e-6 || fabs(1.0 - w) <= 1e-6) ? 0.0 : 1.0; }

__global__ __launch_bounds__(kThreads) void k_gn_robust_resid(GnRobustDev a, const double* __restrict__ u, double* __restrict__ part) {
    __shared__ double red[8];
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const GnDev& d = a.g;
    double r2a = 0.0, r2b = 0.0, nba = 0.0, nbb = 0.0;
    if (i < a.n_a) {
        double r;
        if (a.dim == 2) {
            double xa, ya, xb, yb;
            gn_point(u, d.pin, d.Np, d.rng_a[i], xa, ya);
            gn_point(u, d.pin, d.Np, d.rng_b[i], xb, yb);
            r = gn_range_resid(xa, ya, xb, yb, d.rng_dist[i], a.prec0[i]);
        } else {
            const double* pa = gn_point3(u, d.Np, d.rng_a[i]);
            const double* pb = gn_point3(u, d.Np, d.rng_b[i]);
            const double a3[3] = {pa[0], pa[1], pa[2]}, b3[3] = {pb[0], pb[1], pb[2]};
            r = gn_range_resid3(a3, b3, d.rng_dist[i], a.prec0[i]);
        }
        a.r_rng[i] = r;
        r2a = r == r ? r * r : INFINITY;
        nba = gn_robust_nonbinary(a.w_rng[i]);
    } else if (i < a.n_a + a.n_b) {
        const int64_t e = i - a.n_a, m = a.first_lc + e;
        double r;
        if (a.dim == 2) {
            double thi, xi, yi, thj, xj, yj;
            gn_pose(u, d.pin, d.rel_i[m], thi, xi, yi);
            gn_pose(u, d.pin, d.rel_j[m], thj, xj, yj);
            r = gn_rel_resid(thi, xi, yi, thj, xj, yj, d.rel_t + 2 * m, d.rel_R + 4 * m, a.kappa0[e], a.tau0[e]);
        } else {
            double Xi[12], Xj[12];
            const double* pi = u + 12 * (int64_t)d.rel_i[m];
            const double* pj = u + 12 * (int64_t)d.rel_j[m];
#pragma unroll
            for (int k = 0; k < 12; ++k) { Xi[k] = pi[k]; Xj[k] = pj[k]; }
            r = gn_rel_resid3(Xi, Xj, d.rel_t + 3 * m, d.rel_R + 9 * m, a.kappa0[e], a.tau0[e]);
        }
        a.r_lc[e] = r;
        r2b = r == r ? r * r : INFINITY;
        nbb = gn_robust_nonbinary(a.w_lc[e]);
    }
    r2a = block_max(r2a, red);
    r2b = block_max(r2b, red);
    nba = block_sum(nba, red);
    nbb = block_sum(nbb, red);
    if (threadIdx.x == 0) {
        double* p = part + (int64_t)kGnRobustPart * blockIdx.x;
        p[0] = r2a; p[1] = r2b; p[2] = nba; p[3] = nbb;
    }
}

__global__ __launch_bounds__(kThreads) void k_gn_robust_weight(GnRobustDev a, double mu, double c_rng, double c_lc, double min_weight,
                                                               int apply) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < a.n_a) {
        const double w = mu > 0.0 ? gnc_tls_weight(a.r_rng[i], mu, c_rng) : 1.0;
        a.w_rng[i] = w;
        if (apply) a.prec[i] = a.prec0[i] * fmax(w, min_weight);
    } else if (i < a.n_a + a.n_b) {
        const int64_t e = i - a.n_a, m = a.first_lc + e;
        const double w = mu > 0.0 ? gnc_tls_weight(a.r_lc[e], mu, c_lc) : 1.0;
        a.w_lc[e] = w;
        if (apply) {
            const double f = fmax(w, min_weight);
            a.kappa[m] = a.kappa0[e] * f;
            a.tau[m] = a.tau0[e] * f;
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
inline int64_t gn_n_loop_closures(const GnProblem& P) {  // the trailing n_rel - sum(chain_len - 1) relative-pose entries
    int64_t odom = 0;
    for (int32_t len : P.chain_len) odom += (int64_t)len - 1;
    return P.n_rel() - odom;
}

// mu after the first solve: the smallest c_f^2 / (2 max r_f^2 - c_f^2) of the families with outliers (the most convex start)
inline double gn_robust_mu0(const RobustSeen* seen, int n_seen) {
#pragma clang fp contract(off)
    double mu = 0.0;
    for (const RobustSeen* s = seen; s < seen + n_seen; ++s) {
        const double c2 = s->c * s->c;
        if (!(s->n > 0 && 2.0 * s->r2max > c2)) continue;
        const double m = c2 / (2.0 * s->r2max - c2);
        if (mu == 0.0 || m < mu) mu = m;
    }
    return mu;
}

inline void gn_robust_check(const score_refine_robust_settings& s, const GnProblem& P) {
    auto bad = [](const char* what) { throw std::runtime_error(std::string("score_refine_robust_run: ") + what); };
    if ((s.families & ~(kGnRobustRanges | kGnRobustClosures)) || s.families == 0) bad("families must be 1 (ranges), 2 (loop closures) or 3");
    if (!(std::isfinite(s.inlier_threshold) && s.inlier_threshold > 0.0)) bad("inlier_threshold must be positive and finite");
    if ((s.families & kGnRobustClosures) && !(std::isfinite(s.rel_threshold) && s.rel_threshold > 0.0)) bad("rel_threshold must be positive and finite");
    if (!(std::isfinite(s.mu_step) && s.mu_step > 1.0)) bad("mu_step must be finite and > 1");
    if (!(s.min_weight > 0.0 && s.min_weight <= 1.0)) bad("min_weight must lie in (0, 1]");
    if (s.max_outer < 1) bad("max_outer must be >= 1");
    if (s.inner_iters < 1) bad("inner_iters must be >= 1");
    auto positive = [](double v) { return std::isfinite(v) && v > 0.0; };
    if (s.families & kGnRobustRanges)
        for (double v : P.rng_prec)
            if (!positive(v)) bad("every range precision must be positive and finite");
    if (s.families & kGnRobustClosures) {
        const int64_t n_lc = gn_n_loop_closures(P);
        if (n_lc < 0) bad("fewer relative-pose entries than odometry steps");
        for (int64_t e = P.n_rel() - n_lc; e < P.n_rel(); ++e)
            if (!positive(P.rel_kappa[(size_t)e]) || !positive(P.rel_tau[(size_t)e])) bad("every loop closure's precisions must be positive and finite");
    }
}

struct GnRobustResult {
    int outer_iterations = 0, lm_iterations = 0;
    bool converged = false;
    double mu = 0.0, cost_initial = 0.0;
    GnInfo gi;   // the last run's cost and gradient; linear solves and PCG iterations of all runs
};

// Backend concept: that of gn_levenberg_marquardt, and
//   robust_begin()                         every weight 1, the block kernels' precisions the measured ones
//   int robust_residuals(families, seen)   r of these families at the current point; fills one record per family (ranges first)
//   robust_weights(families, mu)           the weights from the last residuals, the next solve's precisions
template <class Backend>
inline void gn_robust_refine(Backend& be, const score_refine_robust_settings& s, double pcg_rel_tol, GnRobustResult& R) {
    GnInfo& gi = R.gi;
    be.robust_begin();
    gn_levenberg_marquardt(be, s.max_iters, s.tol, pcg_rel_tol, gi);   // solve 1: score_refine_run's
    R.cost_initial = gi.cost_initial;
    R.lm_iterations = gi.iterations;
    int k = 1;
    RobustNext what;
    bool finite = true;
    for (;;) {
        RobustSeen seen[2];
        const int n_seen = be.robust_residuals(s.families, seen);
        what = robust_decide(k, s.max_outer, seen, n_seen);
        for (int f = 0; f < n_seen; ++f) finite = finite && std::isfinite(seen[f].r2max);
        if (what != RobustNext::go) break;
        R.mu = k == 1 ? gn_robust_mu0(seen, n_seen) : R.mu * s.mu_step;
        be.robust_weights(s.families, R.mu);
        ++k;
        gn_levenberg_marquardt(be, s.inner_iters, s.tol, pcg_rel_tol, gi);
        R.lm_iterations += gi.iterations;
    }
    if (k > 1 && finite) {   // the final weights, to max_iters / tol  (not after a solve gone non-finite)
        gn_levenberg_marquardt(be, s.max_iters, s.tol, pcg_rel_tol, gi);
        R.lm_iterations += gi.iterations;
    }
    R.outer_iterations = k;
    R.converged = what == RobustNext::converged;
}

}  // namespace score

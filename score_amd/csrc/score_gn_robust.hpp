// score_gn_robust.hpp -- outlier-robust refinement (include/score_refine_robust.h states the loop in full): GNC-TLS re-weighting
// of the ranges and / or the loop closures on the residuals of the maximum-likelihood cost, around the Levenberg-Marquardt loop
// of score_gn.hpp on one refinement handle.
//
// Device: two streaming kernels, one measurement of the asked families per lane (ranges first, then the loop closures -- the
// trailing relative-pose entries).  What a lane does is stated once for this handle and the group (score_gn_robust_batch.hpp):
//   k_gn_robust_resid   gn_robust_resid_lane: r = gn_robust_residual (score_gn.hpp: the square root of the block functions' own
//                       cost) at the point, with the MEASURED precisions the handle keeps beside the arrays the block kernels read;
//                       per block and family: max r^2 (non-finite r: +inf) and how many weights of this solve are more than 1e-6
//                       from 0 and from 1.  block_max / block_sum only: the host folds the partials in block order (gn_robust_fold).
//   k_gn_robust_weight  gn_robust_weight: w = gnc_tls_weight(r, mu, c_f) (score_robust.hpp, as it stands; mu is an argument,
//                       mu = 0: w = 1) and, in mode kGbrNext, the next solve's precisions prec * max(w, min_weight) into the very
//                       arrays k_gn_blocks reads (rng_prec, rel_kappa, rel_tau): the block kernels stay as they are.
// Host: gn_robust_refine (score_refine_drivers.hpp), a template over the backend concept of gn_lm_run plus three hooks, drives
// the schedule of score_refine_rule.hpp (GncState; its stop rule robust_decide is the relaxation's too).  One device-to-host
// read per outer iteration (the partials) beyond what the LM loop reads.  Here: the settings' checks and the partials' fold.
#pragma once

#include "../../include/score_refine_robust.h"
#include "score_gn_kernels.hpp"
#include "score_robust.hpp"

namespace score {

constexpr int kGnRobustPart = 4;   // doubles per block in the partials: max r^2 (ranges, closures), non-binary weights (ranges, closures)

struct GnRobustArrays {   // ranges in range order, loop closures in loop-closure order (kappa, tau: relative-pose order)
    const double *prec0, *kappa0, *tau0;   // the measured precisions
    double *prec, *kappa, *tau;            // what the block kernels read: rng_prec, rel_kappa, rel_tau
    double *r_rng, *r_lc, *w_rng, *w_lc;   // residuals, weights
};

struct GnRobustDev {
    GnView g;                 // the graph as the block kernels see it, at the point whose residuals are asked for
    int64_t n_a, n_b;         // lanes: ranges [0, n_a), loop closures [n_a, n_a + n_b)  (a family that is not asked for: 0)
    int64_t first_lc;         // loop closure e is relative-pose entry first_lc + e
    GnRobustArrays a;
};

__device__ __forceinline__ double gn_robust_nonbinary(double w) { return (fabs(w) <= 1e-6 || fabs(1.0 - w) <= 1e-6) ? 0.0 : 1.0; }

// One lane of a residual kernel on view v: range i (i < n_a; entry e_rng of the arrays) or loop closure q = i - n_a < n_b
// (entry e_lc of the arrays, relative-pose entry first_lc + q of the view); then the workgroup's four partials into p.
template <int DIM>
__device__ __forceinline__ void gn_robust_resid_lane(const GnView& v, const GnRobustArrays& a, int64_t i, int64_t n_a, int64_t n_b,
                                                     int64_t e_rng, int64_t e_lc, int64_t first_lc, double* red, double* p) {
    double r2a = 0.0, r2b = 0.0, nba = 0.0, nbb = 0.0;
    if (i < n_a) {
        const double r = gn_robust_residual<DIM>(v, kGnRobustRanges, i, a.prec0[e_rng], 0.0);
        a.r_rng[e_rng] = r;
        r2a = r == r ? r * r : INFINITY;
        nba = gn_robust_nonbinary(a.w_rng[e_rng]);
    } else if (i < n_a + n_b) {
        const double r = gn_robust_residual<DIM>(v, kGnRobustClosures, first_lc + (i - n_a), a.kappa0[e_lc], a.tau0[e_lc]);
        a.r_lc[e_lc] = r;
        r2b = r == r ? r * r : INFINITY;
        nbb = gn_robust_nonbinary(a.w_lc[e_lc]);
    }
    r2a = block_max(r2a, red);
    r2b = block_max(r2b, red);
    nba = block_sum(nba, red);
    nbb = block_sum(nbb, red);
    if (threadIdx.x == 0) { p[0] = r2a; p[1] = r2b; p[2] = nba; p[3] = nbb; }
}

// The weight rule on one measurement, by mode: the weight *w from the residual *r (kGbrNext, kGbrInspect: written) or as it
// stands.  Returns the factor on the measurement's measured precisions; the caller stores prec0 * factor in every mode but
// kGbrInspect.
__device__ __forceinline__ double gn_robust_weight(int32_t mode, const double* r, double* w, double mu, double c, double min_weight) {
#pragma clang fp contract(off)
    if (mode == kGbrNext || mode == kGbrInspect) {
        const double wn = mu > 0.0 ? gnc_tls_weight(*r, mu, c) : 1.0;
        *w = wn;
        return fmax(wn, min_weight);
    }
    return mode == kGbrKeep ? *w : 1.0;
}

// (8 waves per SIMD asked for, for one reason only: the kernel with a runtime `dim` that this template replaces ran at that
// occupancy, and the 3-D instance would otherwise come out two registers past it, at 7 -- where k_gbr_resid<3>, the same lane
// function in the group's kernel, has always been and stays)
template <int DIM>
__global__ __launch_bounds__(kThreads, 8) void k_gn_robust_resid(GnRobustDev a, double* __restrict__ part) {
    __shared__ double red[8];
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    gn_robust_resid_lane<DIM>(a.g, a.a, i, a.n_a, a.n_b, i, i - a.n_a, a.first_lc, red, part + (int64_t)kGnRobustPart * blockIdx.x);
}

// mode: kGbrNext (the next solve's precisions are written) or kGbrInspect
__global__ __launch_bounds__(kThreads) void k_gn_robust_weight(GnRobustDev d, double mu, double c_rng, double c_lc, double min_weight,
                                                               int32_t mode) {
#pragma clang fp contract(off)
    const GnRobustArrays& a = d.a;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < d.n_a) {
        const double f = gn_robust_weight(mode, a.r_rng + i, a.w_rng + i, mu, c_rng, min_weight);
        if (mode != kGbrInspect) a.prec[i] = a.prec0[i] * f;
    } else if (i < d.n_a + d.n_b) {
        const int64_t e = i - d.n_a, m = d.first_lc + e;
        const double f = gn_robust_weight(mode, a.r_lc + e, a.w_lc + e, mu, c_lc, min_weight);
        if (mode != kGbrInspect) { a.kappa[m] = a.kappa0[e] * f; a.tau[m] = a.tau0[e] * f; }
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

// the settings of a robust run and the measured precisions of the families they enable (prec: the ranges; kappa, tau: the
// n_lc loop closures); who: the prefix of the message
inline void gn_robust_check_settings(const std::string& who, const score_refine_robust_settings& s, const double* prec, int64_t n_rng,
                                     const double* kappa, const double* tau, int64_t n_lc) {
    auto bad = [&who](const char* what) { throw std::runtime_error(who + what); };
    if ((s.families & ~(kGnRobustRanges | kGnRobustClosures)) || s.families == 0) bad("families must be 1 (ranges), 2 (loop closures) or 3");
    if (!(std::isfinite(s.inlier_threshold) && s.inlier_threshold > 0.0)) bad("inlier_threshold must be positive and finite");
    if ((s.families & kGnRobustClosures) && !(std::isfinite(s.rel_threshold) && s.rel_threshold > 0.0)) bad("rel_threshold must be positive and finite");
    if (!(std::isfinite(s.mu_step) && s.mu_step > 1.0)) bad("mu_step must be finite and > 1");
    if (!(s.min_weight > 0.0 && s.min_weight <= 1.0)) bad("min_weight must lie in (0, 1]");
    if (s.max_outer < 1) bad("max_outer must be >= 1");
    if (s.inner_iters < 1) bad("inner_iters must be >= 1");
    auto positive = [](double v) { return std::isfinite(v) && v > 0.0; };
    if (s.families & kGnRobustRanges)
        for (int64_t e = 0; e < n_rng; ++e)
            if (!positive(prec[e])) bad("every range precision must be positive and finite");
    if (s.families & kGnRobustClosures) {
        if (n_lc < 0) bad("fewer relative-pose entries than odometry steps");
        for (int64_t e = 0; e < n_lc; ++e)
            if (!positive(kappa[e]) || !positive(tau[e])) bad("every loop closure's precisions must be positive and finite");
    }
}
inline void gn_robust_check(const score_refine_robust_settings& s, const GnProblem& P) {
    const int64_t n_lc = gn_n_loop_closures(P), first = P.n_rel() - std::max<int64_t>(n_lc, 0);
    gn_robust_check_settings("score_refine_robust_run: ", s, P.rng_prec.data(), P.n_rng(), P.rel_kappa.data() + first, P.rel_tau.data() + first, n_lc);
}

// the partials of workgroups [b0, b1) of a residual kernel, in workgroup order: per family max r^2 (a NaN: +inf) and the
// count of non-binary weights
inline void gn_robust_fold(const double* part, int b0, int b1, double r2[2], double nonbin[2]) {
    r2[0] = r2[1] = nonbin[0] = nonbin[1] = 0.0;
    for (int b = b0; b < b1; ++b) {
        const double* p = part + (size_t)kGnRobustPart * (size_t)b;
        for (int f = 0; f < 2; ++f) {
            r2[f] = p[f] != p[f] ? INFINITY : std::max(r2[f], p[f]);
            nonbin[f] += p[2 + f];
        }
    }
}

}  // namespace score

// score_refine_rule.hpp -- the rules of the local refinement, stated once and free of HIP: the Levenberg-Marquardt step rule of
// one run, and the GNC-TLS schedule of the runs of an outlier-robust refinement (include/score_refine_robust.h states that loop
// in full).  Both are a state record with its transitions as pure functions: they read and write the record only, and the
// caller does what they ask for.  The drivers (score_refine_drivers.hpp): gn_lm_run / gn_levenberg_marquardt and gb_start /
// gb_round for the step rule, gn_robust_refine and gbr_lock_step for the schedule -- a single handle and a group in lock-step,
// which hold no constant and no decision of their own.  The Python twins are refine._Member and refine_robust._Stage.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/score_refine_robust.h"

namespace score {

// ---------------------------------------------------------------------------
// the Levenberg-Marquardt step rule: lambda0 = 1e-6; x 10 on a failed or non-improving attempt, the run gives up after 12;
// x 0.1 (floor 1e-12) on acceptance; stops on |g|_inf <= tol max(1, f), on a decrease <= 1e-14 max(1, f), after max_iters
// ---------------------------------------------------------------------------
enum LmPhase : int32_t { kLmGradient = 0, kLmSolve = 1, kLmStopped = 2 };

struct LmState {
    double f = 0, lam = 1e-6, gnorm = INFINITY, cost_initial = 0;
    int32_t it = 1, attempts = 0, iterations = 0, linear_solves = 0, pcg_iters = 0;
    LmPhase phase = kLmGradient;
};

inline void lm_stop(LmState& s, int max_iters) {
    s.phase = kLmStopped;
    s.iterations = std::min(s.it, (int32_t)max_iters);
}
// the run starts with cost f at its start point
inline void lm_begin(LmState& s, double f, int max_iters) {
    s = LmState{};
    s.f = s.cost_initial = f;
    if (s.it > max_iters) lm_stop(s, max_iters);
}
// top of iteration s.it: the gradient of the current point is known
inline void lm_after_gradient(LmState& s, double gnorm, double tol, int max_iters) {
    s.gnorm = gnorm;
    if (gnorm <= tol * std::max(1.0, s.f)) { lm_stop(s, max_iters); return; }
    s.attempts = 0;
    s.phase = kLmSolve;
}
// one attempt: the solve (ok, iterations used) and, where it succeeded, the cost at the trial point.  true: the step is
// accepted (the trial point becomes the current one).
inline bool lm_after_solve(LmState& s, bool ok, int used, double fn, int max_iters) {
    s.linear_solves += 1;
    s.pcg_iters += used;
    if (ok && fn < s.f) {
        const double dec = s.f - fn;
        s.f = fn;
        s.lam = std::max(s.lam * 0.1, 1e-12);
        if (dec <= 1e-14 * std::max(1.0, s.f)) { lm_stop(s, max_iters); return true; }
        s.it += 1;
        if (s.it > max_iters) lm_stop(s, max_iters); else s.phase = kLmGradient;
        return true;
    }
    s.lam *= 10.0;
    s.attempts += 1;
    if (s.attempts >= 12) lm_stop(s, max_iters);
    return false;
}

// ---------------------------------------------------------------------------
// GNC-TLS: who stops, and the first mu (the relaxation's loop, score_robust_driver.hpp, decides with robust_decide too)
// ---------------------------------------------------------------------------
constexpr int kGnRobustRanges = 1, kGnRobustClosures = 2;   // the bits of `families`

// what a re-weighted family saw in outer solve k: its items, max r^2, its threshold, the non-binary weights of that solve
struct RobustSeen { int64_t n; double r2max, c; int32_t nonbinary; };
enum class RobustNext { go, converged, gave_up };
inline RobustNext robust_decide(int k, int max_outer, const RobustSeen* seen, int n_seen) {
    bool finite = true, outliers = false;
    int32_t nonbinary = 0;
    for (const RobustSeen* s = seen; s < seen + n_seen; ++s) {
        finite = finite && std::isfinite(s->r2max);
        outliers = outliers || (s->n > 0 && 2.0 * s->r2max > s->c * s->c);
        nonbinary += s->nonbinary;
    }
    if (!finite) return RobustNext::gave_up;                                 // (a solve gone non-finite)
    if (k == 1 ? !outliers : nonbinary == 0) return RobustNext::converged;   // no outliers at all | solved on binary weights
    return k >= max_outer ? RobustNext::gave_up : RobustNext::go;
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

// ---------------------------------------------------------------------------
// the GNC-TLS schedule of a robust refinement: run 1 to max_iters; after a run the residuals, robust_decide, mu and the
// weights, then a run of inner_iters; when the loop stops after a later run on finite residuals, one last run on the final
// weights to max_iters
// ---------------------------------------------------------------------------
enum GncStage : int32_t { kGncFirst = 0, kGncInner = 1, kGncLast = 2, kGncDone = 3 };

struct GncState {
    GncStage stage = kGncFirst;
    int32_t k = 1;                 // outer solves begun
    double mu = 0.0, cost_initial = 0.0;
    bool finite = true, converged = false;
    int32_t lm_iterations = 0, linear_solves = 0, pcg_iters = 0;   // of the runs that have ended
};

struct GncSeen { RobustSeen f[2]; };   // ranges, loop closures: the backend fills n, r2max, nonbinary of both
struct GncNext { bool reweigh, run; };  // new weights from the residuals at R.mu | another run starts

// the iteration cap of the run the state stands in
inline int gnc_run_cap(const GncState& R, const score_refine_robust_settings& s) {
    return R.stage == kGncInner ? s.inner_iters : s.max_iters;
}
// a run has ended: its counters add up.  true: the residuals at its end point are wanted (the last run wants none)
inline bool gnc_run_ended(GncState& R, const LmState& run) {
    if (R.stage == kGncFirst) R.cost_initial = run.cost_initial;
    R.lm_iterations += run.iterations; R.linear_solves += run.linear_solves; R.pcg_iters += run.pcg_iters;
    if (R.stage != kGncLast) return true;
    R.stage = kGncDone;
    return false;
}
// the residuals at the end point of the run are known
inline GncNext gnc_after_residuals(GncState& R, const score_refine_robust_settings& s, const GncSeen& seen) {
    RobustSeen fam[2];
    int n_seen = 0;
    if (s.families & kGnRobustRanges) { fam[n_seen] = seen.f[0]; fam[n_seen++].c = s.inlier_threshold; }
    if (s.families & kGnRobustClosures) { fam[n_seen] = seen.f[1]; fam[n_seen++].c = s.rel_threshold; }
    const RobustNext what = robust_decide(R.k, s.max_outer, fam, n_seen);
    for (int f = 0; f < n_seen; ++f) R.finite = R.finite && std::isfinite(fam[f].r2max);
    if (what == RobustNext::go) {
        R.mu = R.k == 1 ? gn_robust_mu0(fam, n_seen) : R.mu * s.mu_step;
        R.k += 1;
        R.stage = kGncInner;
        return GncNext{true, true};
    }
    R.converged = what == RobustNext::converged;
    const bool last = R.k > 1 && R.finite;   // the final weights, to max_iters / tol  (not after a solve gone non-finite)
    R.stage = last ? kGncLast : kGncDone;
    return GncNext{false, last};
}

}  // namespace score

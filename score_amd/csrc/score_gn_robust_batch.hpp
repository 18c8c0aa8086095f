// score_gn_robust_batch.hpp -- outlier-robust refinement of a GROUP of graphs in lock-step (include/score_refine_robust_batch.h):
// the GNC-TLS outer loop of score_gn_robust.hpp, one per member, around the lock-step Levenberg-Marquardt rounds of
// score_gn_batch.hpp on one group handle.
//
// Device: the two kernels of score_gn_robust.hpp over the union problem.  One measurement per lane, a member's ranges first and
// then its loop closures (its trailing n_lc relative-pose entries), padded at member boundaries (rblk_member, rblk0 / rblk1 of
// GbMember); a workgroup tests its member's mask word first and writes nothing for a member that is masked out.
//   k_gbr_resid    r = gn_range_resid / gn_rel_resid at the member's point in the union state, with the MEASURED precisions
//                  (prec0, kappa0, tau0: arrays of the handle's own, the loop closures in loop-closure order); per workgroup and
//                  family max r^2 (non-finite r: +inf) and the count of non-binary weights.  block_max / block_sum only: the host
//                  folds a member's partials in workgroup order, as a handle on the member alone does.
//   k_gbr_weight   reads the member's GbrParam: w = gnc_tls_weight(r, mu, c_f) (mu = 0: w = 1) in the member's enabled families,
//                  and by `mode` the precisions k_gb_blocks / k_gb_blocks3 read (rng_prec, rel_kappa, rel_tau).
// Host: gbr_lock_step, gb_lock_step plus a stage per member; the decisions are robust_decide and gn_robust_mu0 as they stand.
#pragma once

#include "../../include/score_refine_robust_batch.h"
#include "score_gn_batch.hpp"
#include "score_gn_robust.hpp"

namespace score {

// what k_gbr_weight does with a member
enum GbrMode : int32_t {
    kGbrNext = 0,     // w from r in the enabled families; precisions prec0 * max(w, min_weight) there
    kGbrKeep = 1,     // precisions prec0 * w of the weights as they stand (every family: a family that is off holds w = 1)
    kGbrRestore = 2,  // precisions prec0
    kGbrInspect = 3,  // w from r in the enabled families; the precisions are not touched
};

struct GbrParam {
    double mu, c_rng, c_lc, min_weight;
    int32_t families, mode;
};

struct GbrDev {
    GbDev d;
    const double *prec0, *kappa0, *tau0;   // the measured precisions (kappa0, tau0: loop-closure order)
    double *prec, *kappa, *tau;            // what the block kernels read: rng_prec, rel_kappa, rel_tau
    double *r_rng, *r_lc, *w_rng, *w_lc;   // residuals, weights (ranges as rng_*, loop closures in loop-closure order)
    const GbrParam* params;                // [member]
};

template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gbr_resid(GbrDev a, const double* __restrict__ X, double* __restrict__ part,
                                                        const int32_t* __restrict__ mask) {
    __shared__ double red[8];
    const GbDev& d = a.d;
    const int g = d.rblk_member[blockIdx.x];
    if (!mask[g]) return;
    const GbMember M = d.members[g];
    const double* Xg = X + M.state0;
    const long long i = (long long)((int)blockIdx.x - M.rblk0) * kThreads + threadIdx.x;
    double r2a = 0.0, r2b = 0.0, nba = 0.0, nbb = 0.0;
    if (i < M.n_rng) {
        const long long e = M.rng0 + i;
        const long long va = d.rng_a[e], vb = d.rng_b[e];
        double r;
        if (DIM == 2) {
            const double* pa = va < M.Np ? Xg + 3 * va + 1 : Xg + 3 * M.Np + 2 * (va - M.Np);
            const double* pb = vb < M.Np ? Xg + 3 * vb + 1 : Xg + 3 * M.Np + 2 * (vb - M.Np);
            r = gn_range_resid(pa[0], pa[1], pb[0], pb[1], d.rng_dist[e], a.prec0[e]);
        } else {
            const double* pa = gn_point3(Xg, M.Np, va);
            const double* pb = gn_point3(Xg, M.Np, vb);
            const double a3[3] = {pa[0], pa[1], pa[2]}, b3[3] = {pb[0], pb[1], pb[2]};
            r = gn_range_resid3(a3, b3, d.rng_dist[e], a.prec0[e]);
        }
        a.r_rng[e] = r;
        r2a = r == r ? r * r : INFINITY;
        nba = gn_robust_nonbinary(a.w_rng[e]);
    } else if (i < M.n_rng + M.n_lc) {
        const long long q = i - M.n_rng, e = M.lc0 + q, m = M.rel0 + (M.n_rel - M.n_lc) + q;
        double r;
        if (DIM == 2) {
            const double* pi = Xg + 3 * (long long)d.rel_i[m];
            const double* pj = Xg + 3 * (long long)d.rel_j[m];
            r = gn_rel_resid(pi[0], pi[1], pi[2], pj[0], pj[1], pj[2], d.rel_t + 2 * m, d.rel_R + 4 * m, a.kappa0[e], a.tau0[e]);
        } else {
            double Xi[12], Xj[12];
            const double* pi = Xg + 12 * (long long)d.rel_i[m];
            const double* pj = Xg + 12 * (long long)d.rel_j[m];
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
        double* p = part + (long long)kGnRobustPart * blockIdx.x;
        p[0] = r2a; p[1] = r2b; p[2] = nba; p[3] = nbb;
    }
}

__global__ __launch_bounds__(kThreads) void k_gbr_weight(GbrDev a, const int32_t* __restrict__ mask) {
#pragma clang fp contract(off)
    const GbDev& d = a.d;
    const int g = d.rblk_member[blockIdx.x];
    if (!mask[g]) return;
    const GbMember M = d.members[g];
    const GbrParam p = a.params[g];
    const long long i = (long long)((int)blockIdx.x - M.rblk0) * kThreads + threadIdx.x;
    const bool from_r = p.mode == kGbrNext || p.mode == kGbrInspect;
    if (i < M.n_rng) {
        const long long e = M.rng0 + i;
        if (from_r) {
            if (!(p.families & kGnRobustRanges)) return;
            const double w = p.mu > 0.0 ? gnc_tls_weight(a.r_rng[e], p.mu, p.c_rng) : 1.0;
            a.w_rng[e] = w;
            if (p.mode == kGbrNext) a.prec[e] = a.prec0[e] * fmax(w, p.min_weight);
        } else {
            a.prec[e] = p.mode == kGbrKeep ? a.prec0[e] * a.w_rng[e] : a.prec0[e];
        }
    } else if (i < M.n_rng + M.n_lc) {
        const long long q = i - M.n_rng, e = M.lc0 + q, m = M.rel0 + (M.n_rel - M.n_lc) + q;
        if (from_r) {
            if (!(p.families & kGnRobustClosures)) return;
            const double w = p.mu > 0.0 ? gnc_tls_weight(a.r_lc[e], p.mu, p.c_lc) : 1.0;
            a.w_lc[e] = w;
            if (p.mode == kGbrNext) {
                const double f = fmax(w, p.min_weight);
                a.kappa[m] = a.kappa0[e] * f;
                a.tau[m] = a.tau0[e] * f;
            }
        } else if (p.mode == kGbrKeep) {
            const double w = a.w_lc[e];
            a.kappa[m] = a.kappa0[e] * w;
            a.tau[m] = a.tau0[e] * w;
        } else {
            a.kappa[m] = a.kappa0[e];
            a.tau[m] = a.tau0[e];
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// gn_robust_check on member g's measured precisions (prec: its ranges; kappa, tau: its loop closures)
inline void gbr_check(const score_refine_robust_settings& s, int g, const double* prec, long long n_rng, const double* kappa,
                      const double* tau, long long n_lc) {
    auto bad = [g](const char* what) {
        throw std::runtime_error("score_refine_batch_robust_run: member " + std::to_string(g) + ": " + what);
    };
    if ((s.families & ~(kGnRobustRanges | kGnRobustClosures)) || s.families == 0) bad("families must be 1 (ranges), 2 (loop closures) or 3");
    if (!(std::isfinite(s.inlier_threshold) && s.inlier_threshold > 0.0)) bad("inlier_threshold must be positive and finite");
    if ((s.families & kGnRobustClosures) && !(std::isfinite(s.rel_threshold) && s.rel_threshold > 0.0)) bad("rel_threshold must be positive and finite");
    if (!(std::isfinite(s.mu_step) && s.mu_step > 1.0)) bad("mu_step must be finite and > 1");
    if (!(s.min_weight > 0.0 && s.min_weight <= 1.0)) bad("min_weight must lie in (0, 1]");
    if (s.max_outer < 1) bad("max_outer must be >= 1");
    if (s.inner_iters < 1) bad("inner_iters must be >= 1");
    auto positive = [](double v) { return std::isfinite(v) && v > 0.0; };
    if (s.families & kGnRobustRanges)
        for (long long e = 0; e < n_rng; ++e)
            if (!positive(prec[e])) bad("every range precision must be positive and finite");
    if (s.families & kGnRobustClosures)
        for (long long e = 0; e < n_lc; ++e)
            if (!positive(kappa[e]) || !positive(tau[e])) bad("every loop closure's precisions must be positive and finite");
}

// where member g stands in the schedule of gn_robust_refine
enum GbrStage : int32_t { kGbrFirst = 0, kGbrInner = 1, kGbrLast = 2, kGbrDone = 3 };

struct GbrState {
    GbrStage stage = kGbrFirst;
    int32_t k = 1;                 // outer solves begun
    double mu = 0.0, cost_initial = 0.0;
    bool finite = true, converged = false;
    int32_t lm_iterations = 0, linear_solves = 0, pcg_iters = 0;   // of the runs that have ended
};

struct GbrSeen { RobustSeen f[2]; };   // ranges, loop closures: the backend fills n, r2max, nonbinary

// Backend concept: that of gb_lock_step, and
//   robust_begin()                    every weight 1, the block kernels' precisions the measured ones (all members)
//   robust_residuals(mask, seen)      r of both families of the masked members at their current points; seen[g] per masked member
//   robust_weights(mask, params)      k_gbr_weight on the masked members with params[g]
// Member g follows gn_robust_refine with rs[g]; S[g] is its last run, R[g] the loop around it.  Returns the rounds;
// *stage_rounds: the passes in which some member changed stage.
template <class Backend>
inline int gbr_lock_step(Backend& be, int count, const score_refine_robust_settings* rs, double pcg_rel_tol, std::vector<GbState>& S,
                         std::vector<GbrState>& R, int* stage_rounds) {
    const size_t G = (size_t)count;
    S.assign(G, GbState{});
    R.assign(G, GbrState{});
    GbRoundWork W(G);
    std::vector<char> ended(G), rmask(G), wmask(G), restart(G);
    std::vector<GbrSeen> seen(G);
    std::vector<GbrParam> params(G, GbrParam{});
    auto iters_of = [&](size_t g) { return (int)(R[g].stage == kGbrInner ? rs[g].inner_iters : rs[g].max_iters); };
    auto tol_of = [&](size_t g) { return rs[g].tol; };
    be.robust_begin();
    gb_start(be, S, std::vector<char>(G, 1), iters_of, tol_of, W);   // solve 1: score_refine_batch_run's
    for (size_t g = 0; g < G; ++g) R[g].cost_initial = S[g].cost_initial;
    int rounds = 0, stages = 0;
    for (;;) {
        for (size_t g = 0; g < G; ++g) ended[g] = R[g].stage != kGbrDone && S[g].phase == kGbStopped;
        if (GbRoundWork::any(ended)) {   // the members whose run has just stopped: residuals, decision, mu, weights, next run
            ++stages;
            for (size_t g = 0; g < G; ++g) {
                rmask[g] = wmask[g] = restart[g] = 0;
                if (!ended[g]) continue;
                R[g].lm_iterations += S[g].iterations; R[g].linear_solves += S[g].linear_solves; R[g].pcg_iters += S[g].pcg_iters;
                if (R[g].stage == kGbrLast) R[g].stage = kGbrDone; else rmask[g] = 1;
            }
            if (GbRoundWork::any(rmask)) {
                be.robust_residuals(rmask, seen.data());
                for (size_t g = 0; g < G; ++g) {
                    if (!rmask[g]) continue;
                    const score_refine_robust_settings& s = rs[g];
                    RobustSeen fam[2];
                    int n_seen = 0;
                    if (s.families & kGnRobustRanges) { fam[n_seen] = seen[g].f[0]; fam[n_seen++].c = s.inlier_threshold; }
                    if (s.families & kGnRobustClosures) { fam[n_seen] = seen[g].f[1]; fam[n_seen++].c = s.rel_threshold; }
                    const RobustNext what = robust_decide(R[g].k, s.max_outer, fam, n_seen);
                    for (int f = 0; f < n_seen; ++f) R[g].finite = R[g].finite && std::isfinite(fam[f].r2max);
                    if (what == RobustNext::go) {
                        R[g].mu = R[g].k == 1 ? gn_robust_mu0(fam, n_seen) : R[g].mu * s.mu_step;
                        R[g].k += 1;
                        R[g].stage = kGbrInner;
                        params[g] = GbrParam{R[g].mu, s.inlier_threshold, s.rel_threshold, s.min_weight, s.families, kGbrNext};
                        wmask[g] = restart[g] = 1;
                    } else {
                        R[g].converged = what == RobustNext::converged;
                        if (R[g].k > 1 && R[g].finite) { R[g].stage = kGbrLast; restart[g] = 1; }   // the final weights, to max_iters / tol
                        else R[g].stage = kGbrDone;
                    }
                }
                if (GbRoundWork::any(wmask)) be.robust_weights(wmask, params.data());
            }
            if (GbRoundWork::any(restart)) gb_start(be, S, restart, iters_of, tol_of, W);
            continue;   // (a run may stop where it starts)
        }
        if (!gb_round(be, S, iters_of, tol_of, pcg_rel_tol, W)) break;
        ++rounds;
    }
    if (stage_rounds) *stage_rounds = stages;
    return rounds;
}

}  // namespace score

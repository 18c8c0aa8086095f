// score_gn_robust_batch.hpp -- outlier-robust refinement of a GROUP of graphs in lock-step (include/score_refine_robust_batch.h):
// the GNC-TLS outer loop of score_gn_robust.hpp, one per member, around the lock-step Levenberg-Marquardt rounds of
// score_gn_batch.hpp on one group handle.
//
// Device: the two kernels of score_gn_robust.hpp over the union problem, around the same lane functions.  One measurement per
// lane, a member's ranges first and then its loop closures (its trailing n_lc relative-pose entries), padded at member
// boundaries (rblk_member, rblk0 / rblk1 of GbMember); a workgroup tests its member's mask word first and writes nothing for a
// member that is masked out.
//   k_gbr_resid    gn_robust_resid_lane on the member's view (gb_view): r at the member's point in the union state, with the
//                  MEASURED precisions (prec0, kappa0, tau0: arrays of the handle's own, the loop closures in loop-closure order);
//                  per workgroup and family max r^2 (non-finite r: +inf) and the count of non-binary weights.  The host folds a
//                  member's partials in workgroup order (gn_robust_fold), as a handle on the member alone does.
//   k_gbr_weight   reads the member's GbrParam: gn_robust_weight in the member's enabled families -- w = gnc_tls_weight(r, mu, c_f)
//                  (mu = 0: w = 1) -- and by `mode` the precisions k_gb_blocks reads (rng_prec, rel_kappa, rel_tau).
// Host: gbr_lock_step, gb_lock_step plus a stage per member; the decisions are robust_decide and gn_robust_mu0 as they stand.
#pragma once

#include "../../include/score_refine_robust_batch.h"
#include "score_gn_batch.hpp"
#include "score_gn_robust.hpp"

namespace score {

struct GbrParam {   // what k_gbr_weight does with a member (mode: GbrMode, score_gn_robust.hpp)
    double mu, c_rng, c_lc, min_weight;
    int32_t families, mode;
};

struct GbrDev {
    GbDev d;
    GnRobustArrays a;         // the union's: ranges as rng_*, loop closures in loop-closure order
    const GbrParam* params;   // [member]
};

template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gbr_resid(GbrDev a, const double* __restrict__ X, double* __restrict__ part,
                                                        const int32_t* __restrict__ mask) {
    __shared__ double red[8];
    const GbDev& d = a.d;
    const int g = d.rblk_member[blockIdx.x];
    if (!mask[g]) return;
    const GbMember M = d.members[g];
    const long long i = (long long)((int)blockIdx.x - M.rblk0) * kThreads + threadIdx.x;
    gn_robust_resid_lane<DIM>(gb_view<DIM>(d, M, X, nullptr, nullptr), a.a, i, M.n_rng, M.n_lc, M.rng0 + i, M.lc0 + (i - M.n_rng),
                              M.n_rel - M.n_lc, red, part + (long long)kGnRobustPart * blockIdx.x);
}

__global__ __launch_bounds__(kThreads) void k_gbr_weight(GbrDev d, const int32_t* __restrict__ mask) {
#pragma clang fp contract(off)
    const GnRobustArrays& a = d.a;
    const int g = d.d.rblk_member[blockIdx.x];
    if (!mask[g]) return;
    const GbMember M = d.d.members[g];
    const GbrParam p = d.params[g];
    const long long i = (long long)((int)blockIdx.x - M.rblk0) * kThreads + threadIdx.x;
    const bool from_r = p.mode == kGbrNext || p.mode == kGbrInspect;   // then: in the enabled families only
    if (i < M.n_rng) {
        if (from_r && !(p.families & kGnRobustRanges)) return;
        const long long e = M.rng0 + i;
        const double f = gn_robust_weight(p.mode, a.r_rng + e, a.w_rng + e, p.mu, p.c_rng, p.min_weight);
        if (p.mode != kGbrInspect) a.prec[e] = a.prec0[e] * f;
    } else if (i < M.n_rng + M.n_lc) {
        if (from_r && !(p.families & kGnRobustClosures)) return;
        const long long q = i - M.n_rng, e = M.lc0 + q, m = M.rel0 + (M.n_rel - M.n_lc) + q;
        const double f = gn_robust_weight(p.mode, a.r_lc + e, a.w_lc + e, p.mu, p.c_lc, p.min_weight);
        if (p.mode != kGbrInspect) { a.kappa[m] = a.kappa0[e] * f; a.tau[m] = a.tau0[e] * f; }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// gn_robust_check on member g's measured precisions (prec: its ranges; kappa, tau: its loop closures)
inline void gbr_check(const score_refine_robust_settings& s, int g, const double* prec, long long n_rng, const double* kappa,
                      const double* tau, long long n_lc) {
    gn_robust_check_settings("score_refine_batch_robust_run: member " + std::to_string(g) + ": ", s, prec, n_rng, kappa, tau, n_lc);
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

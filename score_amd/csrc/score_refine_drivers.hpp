// score_refine_drivers.hpp -- the four drivers of the rules of score_refine_rule.hpp, free of HIP: a template over a backend
// each, which do what the rule's transitions ask for and hold no constant and no decision of their own.
//   gn_lm_run          one Levenberg-Marquardt run on a single handle (gn_levenberg_marquardt: the same, into a GnInfo)
//   gb_lock_step       the runs of a group's members in lock-step: gb_start, then gb_round until no member solves
//   gn_robust_refine   the GNC-TLS schedule around gn_lm_run on a single handle
//   gbr_lock_step      the schedule per member around gb_start / gb_round
// The backends are the HIP handles (score_refine_handles.hpp: score_refine, score_refine_batch), the CPU twin's score_refine, and the
// scripted one of tests/tools/refine_rule_check.cpp, which runs every script through all four.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "score_refine_rule.hpp"

namespace score {

// ---------------------------------------------------------------------------
// a single handle: one run
// ---------------------------------------------------------------------------
struct GnInfo {
    double cost_initial = 0, cost_final = 0, grad_inf = 0;
    int32_t iterations = 0, linear_solves = 0, pcg_iters = 0;
};

// what a run leaves in the record: its costs, iterations and last gradient; the solves and PCG iterations add up over runs
inline void gn_info_run(GnInfo& info, const LmState& s) {
    info.cost_initial = s.cost_initial; info.cost_final = s.f; info.grad_inf = s.gnorm;
    info.iterations = s.iterations; info.linear_solves += s.linear_solves; info.pcg_iters += s.pcg_iters;
}

// One Levenberg-Marquardt run from the backend's current point: the step rule is LmState's (score_refine_rule.hpp), this loop
// does what it asks for.  Backend concept:  double eval_current(bool with_blocks) -> cost (and the blocks) at the current
// point;  assemble() -> |g|_inf (g from the blocks of the current point);  bool solve(lambda, rel_tol, &pcg_iters) -> step
// ready (H from the same blocks);  double eval_trial() makes current + step the trial point -> its cost;  accept() makes the
// trial point current.  The blocks of an accepted point are evaluated only when another iteration follows: a run leaves the
// blocks of the last point it took a gradient at, and whoever reads blocks afterwards evaluates first.
template <class Backend>
inline LmState gn_lm_run(Backend& be, int max_iters, double tol, double pcg_rel_tol) {
    LmState s;
    lm_begin(s, be.eval_current(true), max_iters);
    if (s.phase == kLmGradient) lm_after_gradient(s, be.assemble(), tol, max_iters);
    while (s.phase == kLmSolve) {
        int used = 0;
        const bool ok = be.solve(s.lam, pcg_rel_tol, &used);
        const double fn = ok ? be.eval_trial() : NAN;
        if (!lm_after_solve(s, ok, used, fn, max_iters)) continue;
        be.accept();
        if (s.phase != kLmGradient) break;
        (void)be.eval_current(true);
        lm_after_gradient(s, be.assemble(), tol, max_iters);
    }
    return s;
}
template <class Backend>
inline void gn_levenberg_marquardt(Backend& be, int max_iters, double tol, double pcg_rel_tol, GnInfo& info) {
    gn_info_run(info, gn_lm_run(be, max_iters, tol, pcg_rel_tol));
}

// ---------------------------------------------------------------------------
// a group in lock-step: one LmState per member
// ---------------------------------------------------------------------------
// Backend concept (masks: one char per member):
//   eval(mask, trial, with_blocks, cost_or_null)   blocks / cost of the current (or trial) point of the masked members
//   gradient(mask, gnorm)                          g = J'r of the masked members from their blocks, |g|_inf
//   solve(mask, lambda, rel_tol, ok, used)         (J'J + lambda_g I) step = -g for the masked members
//   trial(mask)                                    trial = current + step;     accept(mask)  current = trial
// what a round works with: one entry per member
struct GbRoundWork {
    std::vector<char> mask, tmask, acc, ok;
    std::vector<double> val, lam;
    std::vector<int32_t> used;
    explicit GbRoundWork(size_t G) : mask(G, 1), tmask(G), acc(G), ok(G), val(G, 0.0), lam(G, 0.0), used(G, 0) {}
    static bool any(const std::vector<char>& m) { return std::find(m.begin(), m.end(), (char)1) != m.end(); }
};

// One round: every member in phase kLmSolve gets one damped solve, one trial point and one cost, then decides for itself;
// those that go on get the blocks and the gradient of their new point.  max_iters(g) / tol(g): the limits of member g's run.
// false: no member is in phase kLmSolve (nothing was done).
template <class Backend, class MaxIters, class Tol>
inline bool gb_round(Backend& be, std::vector<LmState>& S, MaxIters max_iters, Tol tol, double pcg_rel_tol, GbRoundWork& W) {
    const size_t G = S.size();
    for (size_t g = 0; g < G; ++g) { W.mask[g] = S[g].phase == kLmSolve; W.lam[g] = S[g].lam; }
    if (!W.any(W.mask)) return false;
    be.solve(W.mask, W.lam.data(), pcg_rel_tol, W.ok.data(), W.used.data());
    for (size_t g = 0; g < G; ++g) W.tmask[g] = W.mask[g] && W.ok[g];
    if (W.any(W.tmask)) {
        be.trial(W.tmask);
        be.eval(W.tmask, true, false, W.val.data());
    }
    for (size_t g = 0; g < G; ++g)
        W.acc[g] = W.mask[g] ? (lm_after_solve(S[g], W.ok[g] != 0, W.used[g], W.val[g], max_iters(g)) ? 1 : 0) : 0;
    if (!W.any(W.acc)) return true;
    be.accept(W.acc);
    for (size_t g = 0; g < G; ++g) W.tmask[g] = W.acc[g] && S[g].phase == kLmGradient;
    if (!W.any(W.tmask)) return true;
    be.eval(W.tmask, false, true, nullptr);
    be.gradient(W.tmask, W.val.data());
    for (size_t g = 0; g < G; ++g)
        if (W.tmask[g]) lm_after_gradient(S[g], W.val[g], tol(g), max_iters(g));
    return true;
}

// The masked members enter a run at their current points: blocks and cost, lm_begin, then the gradient of those that iterate.
template <class Backend, class MaxIters, class Tol>
inline void gb_start(Backend& be, std::vector<LmState>& S, const std::vector<char>& members, MaxIters max_iters, Tol tol, GbRoundWork& W) {
    const size_t G = S.size();
    be.eval(members, false, true, W.val.data());
    for (size_t g = 0; g < G; ++g)
        if (members[g]) lm_begin(S[g], W.val[g], max_iters(g));
    for (size_t g = 0; g < G; ++g) W.tmask[g] = members[g] && S[g].phase == kLmGradient;
    if (!W.any(W.tmask)) return;
    be.gradient(W.tmask, W.val.data());
    for (size_t g = 0; g < G; ++g)
        if (W.tmask[g]) lm_after_gradient(S[g], W.val[g], tol(g), max_iters(g));
}

template <class Backend>
inline int gb_lock_step(Backend& be, int count, int max_iters, double tol, double pcg_rel_tol, std::vector<LmState>& S) {
    const size_t G = (size_t)count;
    S.assign(G, LmState{});
    GbRoundWork W(G);
    auto iters_of = [max_iters](size_t) { return max_iters; };
    auto tol_of = [tol](size_t) { return tol; };
    gb_start(be, S, std::vector<char>(G, 1), iters_of, tol_of, W);
    int rounds = 0;
    while (gb_round(be, S, iters_of, tol_of, pcg_rel_tol, W)) ++rounds;
    return rounds;
}

// ---------------------------------------------------------------------------
// the GNC-TLS schedule: a single handle, a group
// ---------------------------------------------------------------------------
struct GnRobustResult {
    GncState loop;   // outer solves, mu, how it stopped; the counters of all runs
    LmState run;     // the last run: its cost and gradient
};

// The schedule of score_refine_rule.hpp on one handle.  Backend concept: that of gn_lm_run, and
//   robust_begin()                     every weight 1, the block kernels' precisions the measured ones
//   robust_residuals(families, seen)   r of these families at the current point; fills n, r2max, nonbinary of both records
//                                      (ranges, loop closures; a family that is not asked for: zeros)
//   robust_weights(families, mu)       the weights from the last residuals, the next solve's precisions
template <class Backend>
inline void gn_robust_refine(Backend& be, const score_refine_robust_settings& s, double pcg_rel_tol, GnRobustResult& out) {
    GncState& R = out.loop = GncState{};
    be.robust_begin();
    for (;;) {   // run 1 is score_refine_run's
        out.run = gn_lm_run(be, gnc_run_cap(R, s), s.tol, pcg_rel_tol);
        if (!gnc_run_ended(R, out.run)) break;
        GncSeen seen;
        be.robust_residuals(s.families, seen.f);
        const GncNext next = gnc_after_residuals(R, s, seen);
        if (next.reweigh) be.robust_weights(s.families, R.mu);
        if (!next.run) break;
    }
}

// what a weight kernel does with a measurement (the group's k_gbr_weight: by member)
enum GbrMode : int32_t {
    kGbrNext = 0,     // w from r in the enabled families; precisions prec0 * max(w, min_weight) there
    kGbrKeep = 1,     // precisions prec0 * w of the weights as they stand (every family: a family that is off holds w = 1)
    kGbrRestore = 2,  // precisions prec0
    kGbrInspect = 3,  // w from r in the enabled families; the precisions are not touched
};
struct GbrParam {   // what k_gbr_weight does with a member (mode: GbrMode)
    double mu, c_rng, c_lc, min_weight;
    int32_t families, mode;
};

// Backend concept: that of gb_lock_step, and
//   robust_begin()                    every weight 1, the block kernels' precisions the measured ones (all members)
//   robust_residuals(mask, seen)      r of both families of the masked members at their current points; seen[g] (GncSeen) per masked member
//   robust_weights(mask, params)      k_gbr_weight on the masked members with params[g]
// Member g follows the schedule of score_refine_rule.hpp with rs[g] (GncState R[g]; S[g] is its last run), as gn_robust_refine
// follows it on one handle.  Returns the rounds; *stage_rounds: the passes in which some member changed stage.
template <class Backend>
inline int gbr_lock_step(Backend& be, int count, const score_refine_robust_settings* rs, double pcg_rel_tol, std::vector<LmState>& S,
                         std::vector<GncState>& R, int* stage_rounds) {
    const size_t G = (size_t)count;
    S.assign(G, LmState{});
    R.assign(G, GncState{});
    GbRoundWork W(G);
    std::vector<char> ended(G), rmask(G), wmask(G), restart(G);
    std::vector<GncSeen> seen(G);
    std::vector<GbrParam> params(G, GbrParam{});
    auto iters_of = [&](size_t g) { return gnc_run_cap(R[g], rs[g]); };
    auto tol_of = [&](size_t g) { return rs[g].tol; };
    be.robust_begin();
    gb_start(be, S, std::vector<char>(G, 1), iters_of, tol_of, W);   // solve 1: score_refine_batch_run's
    int rounds = 0, stages = 0;
    for (;;) {
        for (size_t g = 0; g < G; ++g) ended[g] = R[g].stage != kGncDone && S[g].phase == kLmStopped;
        if (GbRoundWork::any(ended)) {   // the members whose run has just stopped: residuals, decision, mu, weights, next run
            ++stages;
            for (size_t g = 0; g < G; ++g) {
                wmask[g] = restart[g] = 0;
                rmask[g] = ended[g] && gnc_run_ended(R[g], S[g]);
            }
            if (GbRoundWork::any(rmask)) {
                be.robust_residuals(rmask, seen.data());
                for (size_t g = 0; g < G; ++g) {
                    if (!rmask[g]) continue;
                    const score_refine_robust_settings& s = rs[g];
                    const GncNext next = gnc_after_residuals(R[g], s, seen[g]);
                    if (next.reweigh) params[g] = GbrParam{R[g].mu, s.inlier_threshold, s.rel_threshold, s.min_weight, s.families, kGbrNext};
                    wmask[g] = next.reweigh;
                    restart[g] = next.run;
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

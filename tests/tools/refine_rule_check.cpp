// refine_rule_check.cpp -- the refinement's rules (score_refine_rule.hpp) under their four drivers (score_refine_drivers.hpp) on
// scripted runs: no device, no library.  A script is a table: the cost at the start point, the gradient norms, the verdict,
// iterations used and trial cost of every damped solve, the family records of every residual pass and the cost under every new
// set of weights.  A scripted backend plays the table and logs every lambda passed to `solve`, every mu passed to the weights
// hook and the accepted steps and solves of every run.  (A driver never tells a backend a run's iteration cap; a run that the
// table lets descend for ever ends at its cap, so there the cap is the logged count of steps.)
//
// Every script is run three ways: gn_levenberg_marquardt / gn_robust_refine on a single backend, gb_lock_step / gbr_lock_step
// on a group of one, and the lock-step drivers on a group of two with another script as the second member.  The log and the
// final state must equal the values written by hand below, member for member, all three ways.  Between them the scripts must
// reach every exit of the rules; the program exits non-zero if one was not reached.
//
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I score_amd/csrc refine_rule_check.cpp
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "score_refine_drivers.hpp"

using namespace score;

namespace {

int failures = 0;
void fail(const std::string& where, const std::string& what) {
    std::fprintf(stderr, "FAIL %s: %s\n", where.c_str(), what.c_str());
    ++failures;
}

struct Attempt { bool ok; int used; double fn; };

struct Script {
    std::string name;
    bool robust;
    int max_iters; double tol;                // a plain run
    score_refine_robust_settings rs;          // a robust refinement
    double cost0;
    std::vector<double> gnorm;                // one per gradient
    std::vector<Attempt> attempts;            // one per damped solve
    std::vector<GncSeen> seen;                // one per residual pass
    std::vector<double> reweighed;            // the cost at the current point under each new set of weights
};

struct Log {
    std::vector<double> lam, mu;
    std::vector<int> steps, solves;           // accepted steps and damped solves, per run
    bool operator==(const Log& o) const { return lam == o.lam && mu == o.mu && steps == o.steps && solves == o.solves; }
};

// one scripted graph: the tapes, where they stand, and what was asked of it
struct Sim {
    const Script* sc;
    size_t ig = 0, ia = 0, is = 0, iw = 0;
    double cur, pending = NAN;
    bool overrun = false;
    Log log;
    explicit Sim(const Script& s) : sc(&s), cur(s.cost0) {}
    void run_starts() { log.steps.push_back(0); log.solves.push_back(0); }
    double gradient() {
        if (ig >= sc->gnorm.size()) { overrun = true; return 0.0; }
        return sc->gnorm[ig++];
    }
    Attempt solve(double lam) {
        log.lam.push_back(lam);
        if (log.solves.empty()) overrun = true; else log.solves.back() += 1;
        if (ia >= sc->attempts.size()) { overrun = true; return Attempt{false, 0, NAN}; }
        const Attempt a = sc->attempts[ia++];
        pending = a.fn;
        return a;
    }
    void accept() {
        cur = pending;
        if (log.steps.empty()) overrun = true; else log.steps.back() += 1;
    }
    GncSeen residuals() {
        if (is >= sc->seen.size()) { overrun = true; return GncSeen{}; }
        return sc->seen[is++];
    }
    void weights(double mu) {
        log.mu.push_back(mu);
        if (iw >= sc->reweighed.size()) { overrun = true; return; }
        cur = sc->reweighed[iw++];
    }
    bool played_out() const {
        return !overrun && ig == sc->gnorm.size() && ia == sc->attempts.size() && is == sc->seen.size() && iw == sc->reweighed.size();
    }
};

// the single backend concept (gn_lm_run, gn_robust_refine)
struct Single {
    Sim& m;
    bool boundary = true;   // the next evaluation of the current point opens a run
    double eval_current(bool) {
        if (boundary) m.run_starts();
        boundary = false;
        return m.cur;
    }
    double assemble() { return m.gradient(); }
    bool solve(double lam, double, int* used) {
        const Attempt a = m.solve(lam);
        *used = a.used;
        return a.ok;
    }
    double eval_trial() { return m.pending; }
    void accept() { m.accept(); }
    void robust_begin() {}
    void robust_residuals(int, RobustSeen* seen) {
        const GncSeen s = m.residuals();
        seen[0] = s.f[0]; seen[1] = s.f[1];
        boundary = true;
    }
    void robust_weights(int, double mu) { m.weights(mu); }
};

// the group backend concept (gb_lock_step, gbr_lock_step)
struct Group {
    std::vector<Sim*> m;
    void eval(const std::vector<char>& mask, bool trial, bool, double* cost) {
        for (size_t g = 0; g < m.size(); ++g) {
            if (!mask[g]) continue;
            if (!trial && cost) m[g]->run_starts();   // (gb_start: the only evaluation of current points that asks for the cost)
            if (cost) cost[g] = trial ? m[g]->pending : m[g]->cur;
        }
    }
    void gradient(const std::vector<char>& mask, double* gnorm) {
        for (size_t g = 0; g < m.size(); ++g)
            if (mask[g]) gnorm[g] = m[g]->gradient();
    }
    void solve(const std::vector<char>& mask, const double* lam, double, char* ok, int32_t* used) {
        for (size_t g = 0; g < m.size(); ++g) {
            if (!mask[g]) continue;
            const Attempt a = m[g]->solve(lam[g]);
            ok[g] = a.ok ? 1 : 0;
            used[g] = a.used;
        }
    }
    void trial(const std::vector<char>&) {}
    void accept(const std::vector<char>& mask) {
        for (size_t g = 0; g < m.size(); ++g)
            if (mask[g]) m[g]->accept();
    }
    void robust_begin() {}
    void robust_residuals(const std::vector<char>& mask, GncSeen* seen) {
        for (size_t g = 0; g < m.size(); ++g)
            if (mask[g]) seen[g] = m[g]->residuals();
    }
    void robust_weights(const std::vector<char>& mask, const GbrParam* params) {
        for (size_t g = 0; g < m.size(); ++g) {
            if (!mask[g]) continue;
            const score_refine_robust_settings& s = m[g]->sc->rs;
            if (params[g].mode != kGbrNext || params[g].c_rng != s.inlier_threshold || params[g].c_lc != s.rel_threshold ||
                params[g].min_weight != s.min_weight || params[g].families != s.families)
                m[g]->overrun = true;   // (not the member's own settings)
            m[g]->weights(params[g].mu);
        }
    }
};

// what a script ends in: the last run, and for a robust refinement the loop around the runs
struct Outcome {
    LmState run;
    GncState loop;
    Log log;
    bool played_out = false;
};
bool same(double a, double b) { return a == b || (a != a && b != b); }
bool same_run(const LmState& a, const LmState& b) {
    return same(a.f, b.f) && same(a.gnorm, b.gnorm) && same(a.cost_initial, b.cost_initial) && same(a.lam, b.lam) && a.it == b.it &&
           a.attempts == b.attempts && a.iterations == b.iterations && a.linear_solves == b.linear_solves && a.pcg_iters == b.pcg_iters &&
           a.phase == b.phase;
}
bool same_loop(const GncState& a, const GncState& b) {
    return a.stage == b.stage && a.k == b.k && same(a.mu, b.mu) && same(a.cost_initial, b.cost_initial) && a.finite == b.finite &&
           a.converged == b.converged && a.lm_iterations == b.lm_iterations && a.linear_solves == b.linear_solves &&
           a.pcg_iters == b.pcg_iters;
}

// way 1: the single drivers.  A plain run goes through gn_levenberg_marquardt into a record that already counts 5 solves and
// 7 PCG iterations of earlier runs: those two add up, the rest is overwritten.
Outcome run_single(const Script& sc) {
    Sim sim(sc);
    Single be{sim};
    Outcome o;
    if (sc.robust) {
        GnRobustResult R;
        gn_robust_refine(be, sc.rs, 1e-9, R);
        o.run = R.run; o.loop = R.loop;
    } else {
        GnInfo gi;
        gi.cost_initial = -1; gi.cost_final = -1; gi.grad_inf = -1; gi.iterations = 99; gi.linear_solves = 5; gi.pcg_iters = 7;
        gn_levenberg_marquardt(be, sc.max_iters, sc.tol, 1e-9, gi);
        o.run.cost_initial = gi.cost_initial; o.run.f = gi.cost_final; o.run.gnorm = gi.grad_inf; o.run.iterations = gi.iterations;
        o.run.linear_solves = gi.linear_solves - 5; o.run.pcg_iters = gi.pcg_iters - 7;
    }
    o.log = sim.log;
    o.played_out = sim.played_out();
    return o;
}

// ways 2 and 3: the lock-step drivers on these scripts as one group (all plain or all robust)
std::vector<Outcome> run_group(const std::vector<const Script*>& scs) {
    std::vector<Sim> sims;
    for (const Script* s : scs) sims.emplace_back(*s);
    Group be;
    for (Sim& s : sims) be.m.push_back(&s);
    std::vector<LmState> S;
    std::vector<GncState> R(scs.size());
    if (scs[0]->robust) {
        std::vector<score_refine_robust_settings> rs;
        for (const Script* s : scs) rs.push_back(s->rs);
        int stage_rounds = 0;
        gbr_lock_step(be, (int)scs.size(), rs.data(), 1e-9, S, R, &stage_rounds);
    } else {
        // (gb_lock_step gives every member the same limits; the plain scripts of a pair share theirs)
        gb_lock_step(be, (int)scs.size(), scs[0]->max_iters, scs[0]->tol, 1e-9, S);
    }
    std::vector<Outcome> out(scs.size());
    for (size_t g = 0; g < scs.size(); ++g) {
        out[g].run = S[g]; out[g].loop = R[g]; out[g].log = sims[g].log; out[g].played_out = sims[g].played_out();
    }
    return out;
}

// ---------------------------------------------------------------------------
// the exits the scripts must reach between them
// ---------------------------------------------------------------------------
enum Exit {
    kMaxItersZero, kGradientAtStart, kTwelveRejected, kDecrease, kMaxIters, kGncConvergedFirst, kGncConvergedLater, kGncMaxOuter,
    kGncNonFinite, kRunStopsWhereItStarts, kExits
};
const char* exit_names[kExits] = {"max_iters = 0", "gradient at the start point", "twelve rejected attempts", "the 1e-14 decrease",
                                  "max_iters reached", "GNC converged at k = 1", "GNC converged at k > 1", "max_outer reached",
                                  "non-finite residual", "a run that stops where it starts"};
bool reached[kExits] = {};

void note_exits(const Script& sc, const Outcome& o) {   // o: of a lock-step driver (the whole LmState of the last run)
    const LmState& s = o.run;
    const int cap = sc.robust ? sc.rs.max_iters : sc.max_iters;   // (the last run of every robust script here goes to max_iters)
    const double tol = sc.robust ? sc.rs.tol : sc.tol;
    if (s.phase != kLmStopped) return;
    if (!sc.robust) {
        if (cap == 0 && s.iterations == 0 && s.linear_solves == 0) reached[kMaxItersZero] = true;
        else if (s.it > cap) reached[kMaxIters] = true;
        else if (s.attempts >= 12) {   // the twelve must mix failed solves, worse costs and a NaN cost
            bool failed = false, worse = false, nan = false;
            for (size_t a = sc.attempts.size() - 12; a < sc.attempts.size(); ++a) {
                const Attempt& t = sc.attempts[a];
                failed = failed || !t.ok;
                worse = worse || (t.ok && t.fn >= s.f);
                nan = nan || (t.ok && t.fn != t.fn);
            }
            if (failed && worse && nan) reached[kTwelveRejected] = true;
        } else if (s.gnorm <= tol * std::max(1.0, s.f)) {
            if (s.linear_solves == 0) reached[kGradientAtStart] = true;
        } else reached[kDecrease] = true;
        return;
    }
    const GncState& R = o.loop;
    const size_t runs = o.log.steps.size();
    if (R.stage != kGncDone) return;
    if (R.converged && R.k == 1 && runs == 1) reached[kGncConvergedFirst] = true;
    if (R.converged && R.k > 1 && runs == (size_t)R.k + 1) reached[kGncConvergedLater] = true;
    if (!R.converged && R.finite && R.k >= sc.rs.max_outer && runs == (size_t)R.k + 1) reached[kGncMaxOuter] = true;
    if (!R.converged && !R.finite && runs == (size_t)R.k) reached[kGncNonFinite] = true;
    for (size_t r = 1; r < runs; ++r)   // a later run that finds the gradient small at the point the run before left
        if (o.log.solves[r] == 0 && o.log.steps[r] == 0) reached[kRunStopsWhereItStarts] = true;
}

// ---------------------------------------------------------------------------
// the scripts, and what each must give -- written by hand from the rule as the issue states it
// ---------------------------------------------------------------------------
struct Case { Script sc; Outcome want; };

score_refine_robust_settings settings(int families, double c, double c_rel, double mu_step, int max_outer, int inner_iters, int max_iters) {
    score_refine_robust_settings s;
    s.inlier_threshold = c; s.rel_threshold = c_rel; s.mu_step = mu_step; s.min_weight = 1e-3;
    s.families = families; s.max_outer = max_outer; s.inner_iters = inner_iters; s.max_iters = max_iters; s.tol = 1e-3;
    return s;
}
LmState last_run(double cost_initial, double f, double gnorm, double lam, int it, int attempts, int iterations, int solves, int pcg) {
    LmState s;
    s.cost_initial = cost_initial; s.f = f; s.gnorm = gnorm; s.lam = lam; s.it = it; s.attempts = attempts; s.iterations = iterations;
    s.linear_solves = solves; s.pcg_iters = pcg; s.phase = kLmStopped;
    return s;
}
GncState loop_end(int k, double mu, double cost_initial, bool finite, bool converged, int lm_iterations, int solves, int pcg) {
    GncState R;
    R.stage = kGncDone; R.k = k; R.mu = mu; R.cost_initial = cost_initial; R.finite = finite; R.converged = converged;
    R.lm_iterations = lm_iterations; R.linear_solves = solves; R.pcg_iters = pcg;
    return R;
}
RobustSeen fam(int64_t n, double r2max, int32_t nonbinary) { return RobustSeen{n, r2max, 0.0, nonbinary}; }

std::vector<Case> cases() {
    std::vector<Case> C;
    const double l0 = 1e-6, inf = INFINITY, nan = NAN;
    const score_refine_robust_settings none{};
    // ---- plain runs (pairs share max_iters and tol: P0 + P1, then P2 .. P5) ----
    {   // P0: max_iters = 0: the cost at the start point, nothing else
        Case c{{"P0 max_iters 0", false, 0, 1e-3, none, 5.0, {}, {}, {}, {}}, {}};
        c.want.run = last_run(5.0, 5.0, inf, l0, 1, 0, 0, 0, 0);
        c.want.log = Log{{}, {}, {0}, {0}};
        C.push_back(c);
    }
    {   // P1: max_iters = 0 again, from another cost (the partner of P0)
        Case c{{"P1 max_iters 0", false, 0, 1e-3, none, 0.25, {}, {}, {}, {}}, {}};
        c.want.run = last_run(0.25, 0.25, inf, l0, 1, 0, 0, 0, 0);
        c.want.log = Log{{}, {}, {0}, {0}};
        C.push_back(c);
    }
    {   // P2: |g| = 2e-3 <= tol max(1, f) = 1e-3 * 4 at the start point: no solve, iterations = min(1, 8) = 1
        Case c{{"P2 gradient at start", false, 8, 1e-3, none, 4.0, {2e-3}, {}, {}, {}}, {}};
        c.want.run = last_run(4.0, 4.0, 2e-3, l0, 1, 0, 1, 0, 0);
        c.want.log = Log{{}, {}, {0}, {0}};
        C.push_back(c);
    }
    {   // P3: one accepted step (2 -> 1.5, lambda x 0.1), then twelve rejected attempts (lambda x 10 each): failed solves, worse
        // and equal costs, a NaN cost; gives up in iteration 2
        Case c{{"P3 twelve rejected", false, 8, 1e-3, none, 2.0, {1.0, 0.5},
                {{true, 3, 1.5},
                 {false, 4, 0.0}, {true, 1, 1.6}, {true, 1, nan}, {true, 2, 1.5}, {false, 0, 0.0}, {true, 1, 9.0}, {true, 1, inf},
                 {false, 2, 1.0}, {true, 1, 1.5}, {true, 1, nan}, {true, 1, 2.5}, {true, 1, 1.75}},
                {}, {}}, {}};
        std::vector<double> lam = {l0};
        double l = l0 * 0.1;
        for (int a = 0; a < 12; ++a) { lam.push_back(l); l = l * 10.0; }
        c.want.run = last_run(2.0, 1.5, 0.5, l, 2, 12, 2, 13, 3 + 4 + 1 + 1 + 2 + 0 + 1 + 1 + 2 + 1 + 1 + 1 + 1);
        c.want.log = Log{lam, {}, {1}, {13}};
        C.push_back(c);
    }
    {   // P4: two accepted steps: the first decreases the cost by 2^-46 = 1.42e-14 > 1e-14 max(1, f) and the run goes on, the
        // second by 2^-47 = 7.1e-15 <= 1e-14 max(1, f): stops in iteration 2
        const double f1 = 1.0 - std::ldexp(1.0, -46), f2 = f1 - std::ldexp(1.0, -47);
        Case c{{"P4 decrease", false, 8, 1e-3, none, 1.0, {1.0, 1.0}, {{true, 2, f1}, {true, 1, f2}}, {}, {}}, {}};
        c.want.run = last_run(1.0, f2, 1.0, l0 * 0.1 * 0.1, 2, 0, 2, 2, 3);
        c.want.log = Log{{l0, l0 * 0.1}, {}, {2}, {2}};
        C.push_back(c);
    }
    {   // P5: eight accepted steps: lambda x 0.1 each, never below 1e-12; stops on max_iters = 8
        Case c{{"P5 max_iters", false, 8, 1e-3, none, 256.0, {1, 1, 1, 1, 1, 1, 1, 1},
                {{true, 1, 128}, {true, 1, 64}, {true, 1, 32}, {true, 1, 16}, {true, 1, 8}, {true, 1, 4}, {true, 1, 2}, {true, 1, 1}},
                {}, {}}, {}};
        std::vector<double> lam;
        double l = l0;
        for (int a = 0; a < 8; ++a) { lam.push_back(l); l = l * 0.1 < 1e-12 ? 1e-12 : l * 0.1; }
        if (!(lam[5] > 1e-12 && lam[7] == 1e-12)) fail("P5", "the script does not reach the floor of lambda");
        c.want.run = last_run(256.0, 1.0, 1.0, 1e-12, 9, 0, 8, 8, 8);
        c.want.log = Log{lam, {}, {8}, {8}};
        C.push_back(c);
    }
    // ---- robust refinements: tol = 1e-3; runs that descend for ever show their cap ----
    {   // R0: ranges only; run 1 stops on the gradient at the start point (1e-4 <= 1e-3 * 4); 2 max r^2 = 0.8 <= c^2 = 1: no
        // outlier, converged at k = 1, no further run.  The loop closures' record (off) says otherwise and is not read.
        Case c{{"R0 converged at k = 1", true, 0, 0, settings(1, 1.0, 1.0, 2.0, 5, 2, 3), 4.0, {1e-4}, {},
                {GncSeen{{fam(5, 0.4, 0), fam(3, inf, 2)}}}, {}}, {}};
        c.want.run = last_run(4.0, 4.0, 1e-4, l0, 1, 0, 1, 0, 0);
        c.want.loop = loop_end(1, 0.0, 4.0, true, true, 1, 0, 0);
        c.want.log = Log{{}, {}, {0}, {0}};
        C.push_back(c);
    }
    {   // R1: both families, c = 1, c_rel = 2, mu_step 2, inner_iters 2, max_iters 3.
        //   run 1 (cap 3): 10 -> 6, then |g| = 1e-5 <= 6e-3: iterations 2.  Ranges 2 * 8 > 1: outliers; closures 2 * 2 = 4, not > 4:
        //     none.  mu0 = 1 / (16 - 1) from the ranges alone.
        //   run 2 (cap 2) from cost 5: 5 -> 4.5 -> 4.25, ends at its cap: iterations 2.  One non-binary weight: go, mu x 2.
        //   run 3 (cap 2) from cost 4: |g| = 1e-6 <= 4e-3: stops where it starts, iterations 1.  Binary weights: converged, k = 3.
        //   last run (cap 3) from cost 4: 4 -> 3.5, then |g| = 1e-7: iterations 2.
        Case c{{"R1 converged at k = 3", true, 0, 0, settings(3, 1.0, 2.0, 2.0, 5, 2, 3), 10.0, {1.0, 1e-5, 1.0, 1.0, 1e-6, 0.5, 1e-7},
                {{true, 2, 6.0}, {true, 1, 4.5}, {true, 1, 4.25}, {true, 3, 3.5}},
                {GncSeen{{fam(4, 8.0, 0), fam(2, 2.0, 0)}}, GncSeen{{fam(4, 7.0, 1), fam(2, 1.0, 0)}}, GncSeen{{fam(4, 7.5, 0), fam(2, 1.0, 0)}}},
                {5.0, 4.0}}, {}};
        const double mu0 = 1.0 / 15.0;
        c.want.run = last_run(4.0, 3.5, 1e-7, l0 * 0.1, 2, 0, 2, 1, 3);
        c.want.loop = loop_end(3, mu0 * 2.0, 10.0, true, true, 2 + 2 + 1 + 2, 1 + 2 + 0 + 1, 2 + 1 + 1 + 3);
        c.want.log = Log{{l0, l0, l0 * 0.1, l0}, {mu0, mu0 * 2.0}, {1, 2, 0, 1}, {1, 2, 0, 1}};
        C.push_back(c);
    }
    {   // R2: ranges only, max_outer 2, inner_iters 1, max_iters 3.
        //   run 1 (cap 3): 9 -> 8 -> 7 -> 6, ends at its cap.  2 * 2 > 1: mu0 = 1 / (4 - 1).
        //   run 2 (cap 1) from cost 5: 5 -> 4.5, ends at its cap.  Two non-binary weights, k = 2 = max_outer: gave up, finite.
        //   last run (cap 3) from cost 4.5: -> 4 -> 3.5 -> 3, ends at its cap.
        Case c{{"R2 max_outer", true, 0, 0, settings(1, 1.0, 1.0, 1.5, 2, 1, 3), 9.0, {1, 1, 1, 1, 1, 1, 1},
                {{true, 1, 8.0}, {true, 1, 7.0}, {true, 1, 6.0}, {true, 1, 4.5}, {true, 1, 4.0}, {true, 1, 3.5}, {true, 1, 3.0}},
                {GncSeen{{fam(3, 2.0, 0), fam(0, 0.0, 0)}}, GncSeen{{fam(3, 1.5, 2), fam(0, 0.0, 0)}}}, {5.0}}, {}};
        const double mu0 = 1.0 / 3.0;
        c.want.run = last_run(4.5, 3.0, 1.0, l0 * 0.1 * 0.1 * 0.1, 4, 0, 3, 3, 3);
        c.want.loop = loop_end(2, mu0, 9.0, true, false, 3 + 1 + 3, 7, 7);
        c.want.log = Log{{l0, l0 * 0.1, l0 * 0.1 * 0.1, l0, l0, l0 * 0.1, l0 * 0.1 * 0.1}, {mu0}, {3, 1, 3}, {3, 1, 3}};
        C.push_back(c);
    }
    {   // R3: loop closures only, c_rel = 2.  The ranges' record (off) shows outliers and is not read.
        //   run 1 (cap 3): 7 -> 6 -> 5.5, then |g| = 1e-9: iterations 3.  2 * 50 > 4: mu0 = 4 / (100 - 4).
        //   run 2 (cap 2) from cost 3: a failed solve (lambda x 10), 3 -> 2 -> 1.5, ends at its cap.  max r^2 = inf: gave up on a
        //   non-finite residual, no last run.
        Case c{{"R3 non-finite", true, 0, 0, settings(2, 1.0, 2.0, 1.4, 5, 2, 3), 7.0, {1.0, 1.0, 1e-9, 1.0, 1.0},
                {{true, 1, 6.0}, {true, 2, 5.5}, {false, 5, 0.0}, {true, 1, 2.0}, {true, 1, 1.5}},
                {GncSeen{{fam(9, 1e9, 0), fam(2, 50.0, 0)}}, GncSeen{{fam(9, 1e9, 0), fam(2, inf, 1)}}}, {3.0}}, {}};
        const double mu0 = 4.0 / 96.0;
        c.want.run = last_run(3.0, 1.5, 1.0, l0 * 10.0 * 0.1 * 0.1, 3, 0, 2, 3, 7);
        c.want.loop = loop_end(2, mu0, 7.0, false, false, 3 + 2, 2 + 3, 3 + 7);
        c.want.log = Log{{l0, l0 * 0.1, l0, l0 * 10.0, l0 * 10.0 * 0.1}, {mu0}, {2, 2}, {2, 3}};
        C.push_back(c);
    }
    return C;
}

void check(const std::string& where, const Case& c, const Outcome& got, bool whole_run) {
    if (!got.played_out) fail(where, "the script was not played to its end, or past it");
    if (!(got.log == c.want.log)) fail(where, "the lambdas, mus or steps per run differ from the hand-written ones");
    const LmState& w = c.want.run;
    const LmState& g = got.run;
    if (whole_run ? !same_run(g, w)
                  : !(same(g.cost_initial, w.cost_initial) && same(g.f, w.f) && same(g.gnorm, w.gnorm) && g.iterations == w.iterations &&
                      g.linear_solves == w.linear_solves && g.pcg_iters == w.pcg_iters))
        fail(where, "the last run's state differs from the hand-written one");
    if (c.sc.robust && !same_loop(got.loop, c.want.loop)) fail(where, "the loop's state differs from the hand-written one");
}

}  // namespace

int main() {
    const std::vector<Case> C = cases();
    // the second member of a script's group of two: plain scripts pair within the same limits, robust ones with the next
    const int partner[] = {1, 0, 3, 4, 5, 2, 7, 8, 9, 6};
    for (size_t i = 0; i < C.size(); ++i) {
        const Case& c = C[i];
        const Outcome one = run_single(c.sc);
        check(c.sc.name + " / single", c, one, c.sc.robust);
        const Outcome alone = run_group({&c.sc})[0];
        check(c.sc.name + " / group of one", c, alone, true);
        const Case& p = C[(size_t)partner[i]];
        const std::vector<Outcome> two = run_group({&c.sc, &p.sc});
        check(c.sc.name + " / group of two", c, two[0], true);
        check(p.sc.name + " / group of two, second member", p, two[1], true);
        if (!(one.log == alone.log && alone.log == two[0].log)) fail(c.sc.name, "the three ways do not log the same");
        note_exits(c.sc, alone);
    }
    for (int e = 0; e < kExits; ++e)
        if (!reached[e]) fail("exits", std::string("no script reached: ") + exit_names[e]);
    if (failures) return 1;
    std::printf("refine_rule_check: %zu scripts, three ways each, every exit reached\n", C.size());
    return 0;
}

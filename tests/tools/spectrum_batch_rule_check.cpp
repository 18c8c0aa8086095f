// spectrum_batch_rule_check.cpp -- the mode rule of score_spectrum_batch_rule.hpp driven through scripted norm sequences,
// stand-alone (tests/test_spectrum_batch_host.py builds it with the host sanitizers and runs it as a child process; it is
// never loaded into Python and needs no GPU).  Every script lists, round by round, what the driver would read -- the norm of
// the member's k columns and the status of its last Rayleigh-Ritz step -- and the state the rule must leave, written by
// hand below.  It exits non-zero on the first difference, and unless the scripts reach every exit of the rule.
#include <cstdio>
#include <cmath>
#include <vector>

#include "score_spectrum_batch_rule.hpp"

using namespace score;

namespace {

constexpr double kTol = 1e-3, kAbove = 1.0, kBelow = 1e-4;
constexpr int kK = 4;
int failures = 0;
bool reached[8] = {};  // exits of the rule, see main

struct Round {
    double norm;      // of every one of the k columns (the other 12 are far above tolerance)
    int ritz;         // status of the last Rayleigh-Ritz step: 0 ok, 1 without P, 2 breakdown
    GspMode mode;     // what the rule must leave
    int iterations;
    bool has_p;
};

void expect(bool ok, const char* script, int round, const char* what) {
    if (ok) return;
    std::fprintf(stderr, "%s, round %d: %s\n", script, round, what);
    ++failures;
}

GspState run(const char* script, const std::vector<Round>& rounds, int max_iters) {
    GspState s;
    gsp_begin(s);
    expect(s.mode == kGspIterate && s.ritz_pending && !s.has_p && gsp_word(s) == 0, script, -1, "the start");
    int r = 0;
    for (const Round& q : rounds) {
        double norms[16];
        for (int c = 0; c < 16; ++c) norms[c] = c < kK ? q.norm : 1e3;
        expect(gsp_live(s), script, r, "a member that has ended is read again");
        const GspState before = s;
        gsp_after_residual(s, norms, kK, kTol, q.ritz, max_iters);
        expect(s.mode == q.mode, script, r, "mode");
        expect(s.iterations == q.iterations, script, r, "iterations");
        expect(s.has_p == q.has_p, script, r, "has_p");
        expect(gsp_word(s) == ((int)q.mode | (q.has_p ? 256 : 0)), script, r, "control word");
        expect(s.ritz_pending == (s.mode == kGspIterate), script, r, "a Rayleigh-Ritz step is pending exactly where the second half runs");
        if (before.mode == kGspIterate && s.mode == kGspVerify && !s.last) reached[0] = true;   // done by the recurrence
        if (before.mode == kGspVerify && s.mode == kGspIterate) reached[1] = true;              // ... but not by the product
        if (before.mode == kGspVerify && s.mode == kGspFinished && s.converged) reached[2] = true;
        if (before.mode == kGspIterate && s.mode == kGspVerify && s.last && !s.broke) reached[3] = true;  // the cap
        if (before.mode == kGspVerify && s.mode == kGspFinished && !s.converged) reached[4] = true;       // ... and its verdict
        if (before.mode == kGspIterate && s.mode == kGspVerify && s.broke) reached[5] = true;
        if (s.mode == kGspBroken) reached[6] = true;
        if (before.mode == kGspVerify && s.mode == kGspFinished && s.converged && s.last) reached[7] = true;  // converged at the cap
        ++r;
    }
    return s;
}

}  // namespace

int main() {
    // a plain run: the start block's step is no iteration; three steps, done by the recurrence, done by the product
    {
        GspState s = run("plain", {{kAbove, 0, kGspIterate, 0, false}, {kAbove, 0, kGspIterate, 1, true}, {kAbove, 1, kGspIterate, 2, true},
                                   {kBelow, 0, kGspVerify, 3, true}, {kBelow, 0, kGspFinished, 3, true}}, 200);
        expect(s.converged && gsp_reported_iterations(s) == 3, "plain", 5, "the report");
    }
    // done by the recurrence but not by the product: back to iterating in the same round, then done by both
    {
        GspState s = run("drift", {{kAbove, 0, kGspIterate, 0, false}, {kBelow, 0, kGspVerify, 1, true}, {kAbove, 0, kGspIterate, 1, true},
                                   {kBelow, 0, kGspVerify, 2, true}, {kBelow, 0, kGspFinished, 2, true}}, 200);
        expect(s.converged && gsp_reported_iterations(s) == 2, "drift", 5, "the report");
    }
    // the cap reached: one last verification, whose verdict ends the member either way
    {
        GspState s = run("cap", {{kAbove, 0, kGspIterate, 0, false}, {kAbove, 0, kGspIterate, 1, true}, {kAbove, 0, kGspVerify, 2, true},
                                 {kAbove, 0, kGspFinished, 2, true}}, 2);
        expect(!s.converged && gsp_reported_iterations(s) == -3, "cap", 4, "the report");
        s = run("cap, then converged by the product", {{kAbove, 0, kGspIterate, 0, false}, {kBelow, 0, kGspVerify, 1, true},
                                                       {kBelow, 0, kGspFinished, 1, true}}, 1);
        expect(s.converged && s.last && gsp_reported_iterations(s) == 1, "cap, then converged", 3, "the report");
        // the cap reached while verifying: sent back by the product at iteration 1 of 2, the next step is the last
        s = run("cap while verifying", {{kAbove, 0, kGspIterate, 0, false}, {kBelow, 0, kGspVerify, 1, true}, {kAbove, 0, kGspIterate, 1, true},
                                        {kBelow, 0, kGspVerify, 2, true}, {kAbove, 0, kGspFinished, 2, true}}, 2);
        expect(!s.converged && s.last && gsp_reported_iterations(s) == -3, "cap while verifying", 5, "the report");
    }
    // breakdown: at the start block, and in an iteration (the step is not counted); the member ends broken whatever the norms
    {
        GspState s = run("breakdown at the start", {{kAbove, 2, kGspVerify, 0, false}, {kAbove, 0, kGspBroken, 0, false}}, 200);
        expect(!s.converged && gsp_reported_iterations(s) == -1, "breakdown at the start", 2, "the report");
        s = run("breakdown", {{kAbove, 0, kGspIterate, 0, false}, {kAbove, 0, kGspIterate, 1, true}, {kAbove, 2, kGspVerify, 1, true},
                              {kBelow, 0, kGspBroken, 1, true}}, 200);
        expect(!s.converged && s.broke && gsp_reported_iterations(s) == -2, "breakdown", 4, "the report");
    }
    // a member finished while others go on: the driver no longer reads it, and its state stands
    {
        GspState early = run("early", {{kBelow, 0, kGspVerify, 0, false}, {kBelow, 0, kGspFinished, 0, false}}, 200);
        GspState late = run("late", {{kAbove, 0, kGspIterate, 0, false}, {kAbove, 0, kGspIterate, 1, true}, {kAbove, 0, kGspIterate, 2, true}}, 200);
        const GspState kept = early;
        double norms[16];
        for (double& v : norms) v = kAbove;
        gsp_after_residual(early, norms, kK, kTol, 2, 200);  // (a stray call changes nothing)
        expect(!gsp_live(early) && early.mode == kept.mode && early.iterations == kept.iterations && early.converged == kept.converged &&
                   early.has_p == kept.has_p && early.ritz_pending == kept.ritz_pending && early.last == kept.last &&
                   early.broke == kept.broke && early.started == kept.started,
               "early", 2, "a finished member is left as it is");
        expect(gsp_live(late) && late.iterations == 2 && gsp_reported_iterations(early) == 0, "late", 3, "the others go on");
    }
    // a non-finite norm is not done
    {
        double norms[16];
        for (double& v : norms) v = kBelow;
        norms[2] = std::nan("");
        expect(!gsp_first_k_done(norms, kK, kTol) && gsp_first_k_done(norms, 2, kTol), "nan", 0, "gsp_first_k_done");
    }
    for (int e = 0; e < 8; ++e)
        if (!reached[e]) { std::fprintf(stderr, "exit %d of the rule was not reached\n", e); ++failures; }
    if (failures) return 1;
    std::printf("every exit reached\n");
    return 0;
}

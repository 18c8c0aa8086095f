// score_leverage_batch_plan.hpp -- the HIP-free part of the batched range leverage and predicted range variances
// (include/score_leverage_batch.h): the argument checks on the members' pair lists, where every member's measurement sums and
// pair outputs start, the member of every listed pair, and -- for the range variances -- the pass and slot that solve a
// (member, pair) and the slots (NV) of a pass.  The draws' own plan is score_samples_batch_plan.hpp's (gbs_plan): the
// leverage call is that plan plus this one.  score_leverage_batch.hpp drives the device by it;
// tests/tools/leverage_batch_plan_check.cpp walks it against tables written by hand, stand-alone under the host sanitizers.
//
// Pair pass k of width W solves pair k W + c of EVERY member in slot c; a member with C_g <= k W has dropped out.
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "score_samples_batch_plan.hpp"

namespace score {

// what the plan needs of a member: its variables (poses + landmarks: the ids a pair may name) and its measurements
struct GblShape {
    int64_t vars, meas;
};

struct GblPlan {
    int G = 0, W = 0, passes = 0, most = 0;  // members, width, pair passes, the largest C_g
    int64_t pairs = 0, meas = 0;             // all listed pairs; the measurements of the whole group (the device's stride)
    std::vector<int32_t> pair_ptr;           // [g + 1] prefix sums of C_g (zeros without lists): what the device reads
    std::vector<int32_t> pair_member;        // [pair] its member
    std::vector<int64_t> meas0;              // [g] where member g's sums start in the device's buffers (every member has room)
    std::vector<int64_t> meas_off;           // [g + 1] where they start in lev_sum .. red_sq (members that take part only)

    int count(int g) const { return (int)(pair_ptr[(size_t)g + 1] - pair_ptr[(size_t)g]); }
    // live slots of member g in pair pass k
    int live(int g, int k) const { return std::max(0, std::min(W, count(g) - k * W)); }
    // the pass and the slot that solve pair p (an index into pair_a / pair_b)
    int pass_of(int64_t p) const { return (int)((p - pair_ptr[(size_t)pair_member[(size_t)p]]) / W); }
    int slot_of(int64_t p) const { return (int)((p - pair_ptr[(size_t)pair_member[(size_t)p]]) % W); }
    // the pair in slot c of member g in pass k (-1: the slot carries none)
    int64_t pair_at(int g, int c, int k) const { return c >= 0 && c < live(g, k) ? (int64_t)pair_ptr[(size_t)g] + k * W + c : -1; }
    // slots of pass k
    int nv(int k) const {
        int top = 0;
        for (int g = 0; g < G; ++g) top = std::max(top, live(g, k));
        return gbs_slots(top);
    }
};

// The plan of a call, checked.  who: the entry point's name with ": ".  n_samples: the members' draw counts (the leverage:
// a member without draws may list no pair and has no room in the sums) or null (the range variances: every member takes
// part).  pair_ptr null: no pairs for anyone.
inline GblPlan gbl_plan(const std::string& who, int G, int32_t block_width, const int32_t* n_samples, const std::vector<GblShape>& shapes,
                        const int32_t* pair_ptr, const int32_t* pair_a, const int32_t* pair_b) {
    if (G < 1) throw std::runtime_error(who + "no members");
    if (block_width < 1 || block_width > kGbsMaxWidth) throw std::runtime_error(who + "block_width must be 1..16");
    GblPlan p;
    p.G = G; p.W = block_width;
    p.pair_ptr.assign((size_t)G + 1, 0);
    p.meas_off.assign(1, 0);
    if (pair_ptr && pair_ptr[0] != 0) throw std::runtime_error(who + "pair_ptr must start at 0");
    for (int g = 0; pair_ptr && g < G; ++g)  // (the offsets before anything is read through them)
        if (pair_ptr[g + 1] < pair_ptr[g]) throw std::runtime_error(who + "pair_ptr must not decrease");
    for (int g = 0; g < G; ++g) {
        const GblShape& s = shapes[(size_t)g];
        const std::string member = who + "member " + std::to_string(g) + ": ";
        const bool takes_part = !n_samples || n_samples[g] > 0;
        p.meas0.push_back(p.meas);
        p.meas += s.meas;
        p.meas_off.push_back(p.meas_off.back() + (takes_part ? s.meas : 0));
        if (!pair_ptr) continue;
        const int32_t cnt = pair_ptr[g + 1] - pair_ptr[g];
        p.pair_ptr[(size_t)g + 1] = pair_ptr[g + 1];
        if (cnt == 0) continue;
        if (!(pair_a && pair_b)) throw std::runtime_error(who + "pairs without their lists");
        if (!takes_part) throw std::runtime_error(member + "pairs listed for a member without draws");
        for (int32_t c = pair_ptr[g]; c < pair_ptr[g + 1]; ++c) {
            const int64_t a = pair_a[c], b = pair_b[c];
            if (a < 0 || a >= s.vars || b < 0 || b >= s.vars) throw std::runtime_error(member + "a pair's variable is out of range");
            if (a == b) throw std::runtime_error(member + "a pair joins a variable to itself");
            p.pair_member.push_back(g);
        }
        p.most = std::max(p.most, (int)cnt);
    }
    p.pairs = (int64_t)p.pair_member.size();
    p.passes = (p.most + p.W - 1) / p.W;
    return p;
}

}  // namespace score

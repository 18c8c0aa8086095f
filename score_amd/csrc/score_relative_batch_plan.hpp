// score_relative_batch_plan.hpp -- the HIP-free part of the batched predicted relative poses
// (include/score_relative_batch.h): the argument checks on the members' pair lists, the prefix sums of the members' COLUMNS
// the device reads, the member of every listed pair, and the pass and slot that solve a (member, column).
// score_relative_batch.hpp drives the device by it; tests/tools/relative_batch_plan_check.cpp walks it against tables written
// by hand, stand-alone under the host sanitizers.
//
// Member g with C_g pairs has K_g = DP C_g columns; column j = c DP + q solves H_g x_j = G_c'e_q.  Pass k of width W carries
// column k W + s of EVERY member in slot s; a member with K_g <= k W has dropped out.  Unlike the ranges' plan
// (score_leverage_batch_plan.hpp: one pair, one column) a pair is DP consecutive columns and may straddle two passes.
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "score_samples_batch_plan.hpp"

namespace score {

// the pair and the error coordinate a slot solves (pair -1: the slot carries no column)
struct GrpColumn {
    int64_t pair;
    int q;
};

struct GrpPlan {
    int G = 0, W = 0, DP = 3, passes = 0;
    int64_t most = 0;                  // the largest K_g
    int64_t pairs = 0, columns = 0;    // all listed pairs and their columns
    std::vector<int32_t> pair_ptr;     // [g + 1] prefix sums of C_g (zeros without lists)
    std::vector<int32_t> col_ptr;      // [g + 1] DP * pair_ptr: what the device reads (GbmArgs::sel_ptr, GbsArgs::cnt_ptr)
    std::vector<int32_t> pair_member;  // [pair] its member

    int64_t count(int g) const { return (int64_t)col_ptr[(size_t)g + 1] - col_ptr[(size_t)g]; }  // K_g
    // live slots of member g in pass k
    int live(int g, int k) const { return (int)std::max<int64_t>(0, std::min<int64_t>(W, count(g) - (int64_t)k * W)); }
    // what slot s of member g solves in pass k: global column col_ptr[g] + k W + s is pair / DP, coordinate % DP
    GrpColumn column_at(int g, int s, int k) const {
        if (s < 0 || s >= live(g, k)) return GrpColumn{-1, 0};
        const int64_t j = (int64_t)col_ptr[(size_t)g] + (int64_t)k * W + s;
        return GrpColumn{j / DP, (int)(j % DP)};
    }
    // slots of pass k
    int nv(int k) const {
        int top = 0;
        for (int g = 0; g < G; ++g) top = std::max(top, live(g, k));
        return gbs_slots(top);
    }
};

// The plan of a call, checked.  who: the entry point's name with ": ".  n_poses: Np_g of every member (the ids a pair may
// name).  pair_ptr null: no pairs for anyone.
inline GrpPlan grp_plan(const std::string& who, int G, int dp, int32_t block_width, const std::vector<int64_t>& n_poses,
                        const int32_t* pair_ptr, const int32_t* pair_a, const int32_t* pair_b) {
    if (G < 1) throw std::runtime_error(who + "no members");
    if (block_width < 1 || block_width > kGbsMaxWidth) throw std::runtime_error(who + "block_width must be 1..16");
    GrpPlan p;
    p.G = G; p.W = block_width; p.DP = dp;
    p.pair_ptr.assign((size_t)G + 1, 0);
    p.col_ptr.assign((size_t)G + 1, 0);
    if (!pair_ptr) return p;
    if (pair_ptr[0] != 0) throw std::runtime_error(who + "pair_ptr must start at 0");
    for (int g = 0; g < G; ++g)  // (the offsets before anything is read through them)
        if (pair_ptr[g + 1] < pair_ptr[g]) throw std::runtime_error(who + "pair_ptr must not decrease");
    // (rp_check_pairs' guard on the group's total: the columns and a pair's DP x DP block are indexed through int32 sums)
    if ((long long)pair_ptr[G] * 36 > INT32_MAX) throw std::runtime_error(who + "too many pairs for one call");
    if (pair_ptr[G] > 0 && !(pair_a && pair_b)) throw std::runtime_error(who + "pairs without their lists");
    for (int g = 0; g < G; ++g) {
        const std::string member = who + "member " + std::to_string(g) + ": ";
        const int64_t np = n_poses[(size_t)g];
        p.pair_ptr[(size_t)g + 1] = pair_ptr[g + 1];
        p.col_ptr[(size_t)g + 1] = (int32_t)(dp * pair_ptr[g + 1]);
        for (int32_t c = pair_ptr[g]; c < pair_ptr[g + 1]; ++c) {
            const int64_t a = pair_a[c], b = pair_b[c];
            if (a < 0 || a >= np || b < 0 || b >= np)
                throw std::runtime_error(member + "a pair's pose is out of range (a landmark has no relative pose)");
            if (a == b) throw std::runtime_error(member + "a pair joins a pose to itself");
            p.pair_member.push_back(g);
        }
        p.most = std::max(p.most, p.count(g));
    }
    p.pairs = (int64_t)p.pair_member.size();
    p.columns = p.pairs * dp;
    p.passes = (int)((p.most + p.W - 1) / p.W);
    return p;
}

}  // namespace score

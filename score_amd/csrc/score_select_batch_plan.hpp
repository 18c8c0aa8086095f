// score_select_batch_plan.hpp -- the HIP-free part of the batched greedy selection of candidate ranges
// (include/score_select_batch.h): the argument checks on the members' picks and precisions, where every member's block of P,
// of L and of the picks starts, the table that maps a workgroup of the symmetrisation to (member, tile pair), and the members
// that have candidates (one workgroup of the factorisation each).  The pairs' own plan -- pair_ptr checked, a pair's member,
// pass and slot -- is score_leverage_batch_plan.hpp's (gbl_plan): the selection call is that plan plus this one.
// score_select_batch.hpp drives the device by it; tests/tools/select_batch_plan_check.cpp walks it against tables written by
// hand, stand-alone under the host sanitizers.
//
// Member g with C_g candidates and k_g picks has P_g (C_g x C_g, row-major) at mat0[g], L_g (C_g x k_g, column j at j C_g) at
// l0[g] and its picks at pick0[g].  Its T_g = ceil(C_g / 32) tiles a side give T_g (T_g + 1) / 2 tile pairs (i, j), i <= j,
// row by row: workgroups wg0[g] .. wg0[g + 1] of the symmetrisation.
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "score_select_rule.hpp"

namespace score {

constexpr int kGbSelTile = 32;                            // kSelTile of score_select.hpp
constexpr int64_t kGbSelMaxEntries = (int64_t)1 << 28;    // of all members' P: 2 GiB

struct GbSelTilePair {
    int32_t member, i, j;
};

struct GbSelPlan {
    int G = 0;
    int64_t pairs = 0, entries = 0, l_entries = 0;
    int32_t picks = 0;                    // the sum of k_g
    std::vector<int32_t> count, k;        // [g] C_g, k_g
    std::vector<int64_t> mat0, l0;        // [g + 1]
    std::vector<int32_t> pick0, wg0;      // [g + 1]
    std::vector<GbSelTilePair> tile;      // [workgroup of the symmetrisation]
    std::vector<int32_t> active;          // the members with candidates, ascending
    int tiles(int g) const { return (count[(size_t)g] + kGbSelTile - 1) / kGbSelTile; }
};

// The plan of a call, checked.  who: the entry point's name with ": ".  pair_ptr: G + 1 prefix sums of C_g, already checked
// (GblPlan::pair_ptr).  precisions: one per listed pair; k: one per member.
inline GbSelPlan gbsel_plan(const std::string& who, int G, const std::vector<int32_t>& pair_ptr, const double* precisions, const int32_t* k,
                            double min_gain) {
    if (G < 1 || pair_ptr.size() != (size_t)G + 1) throw std::runtime_error(who + "no members");
    GbSelPlan p;
    p.G = G;
    p.pairs = pair_ptr[(size_t)G];
    p.mat0.assign(1, 0); p.l0.assign(1, 0); p.pick0.assign(1, 0); p.wg0.assign(1, 0);
    if (!(min_gain >= 0.0)) throw std::runtime_error(who + "min_gain must be >= 0");
    if (p.pairs > 0 && !k) throw std::runtime_error(who + "k is missing");
    if (p.pairs > 0 && !precisions) throw std::runtime_error(who + "the precisions are missing");
    for (int g = 0; g < G; ++g) {
        const std::string member = who + "member " + std::to_string(g) + ": ";
        const int32_t C = pair_ptr[(size_t)g + 1] - pair_ptr[(size_t)g], kg = k ? k[g] : 0;
        if (C > kSelMaxCandidates) throw std::runtime_error(member + "the number of candidates must be at most 4096");
        if (C == 0 && kg != 0) throw std::runtime_error(member + "k must be 0 for a member without candidates");
        if (C > 0 && (kg < 1 || kg > kSelMaxPicks || kg > C)) throw std::runtime_error(member + "k must be 1..min(candidates, 256)");
        for (int32_t c = pair_ptr[(size_t)g]; c < pair_ptr[(size_t)g + 1]; ++c)
            if (!(precisions[c] > 0.0) || !std::isfinite(precisions[c])) throw std::runtime_error(member + "a precision must be finite and positive");
        p.count.push_back(C); p.k.push_back(kg);
        p.mat0.push_back(p.mat0.back() + (int64_t)C * C);
        p.l0.push_back(p.l0.back() + (int64_t)C * kg);
        p.pick0.push_back(p.pick0.back() + kg);
        const int T = p.tiles(g);
        for (int i = 0; i < T; ++i)
            for (int j = i; j < T; ++j) p.tile.push_back(GbSelTilePair{g, i, j});
        p.wg0.push_back((int32_t)p.tile.size());
        if (C > 0) p.active.push_back(g);
    }
    p.entries = p.mat0.back(); p.l_entries = p.l0.back(); p.picks = p.pick0.back();
    if (p.entries > kGbSelMaxEntries)
        throw std::runtime_error(who + "the members' matrices take " + std::to_string(p.entries) + " entries: at most 268435456 (2^28, 2 GiB) in one call");
    return p;
}

}  // namespace score

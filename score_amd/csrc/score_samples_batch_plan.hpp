// score_samples_batch_plan.hpp -- the HIP-free part of the batched posterior samples (include/score_samples_batch.h): the
// argument checks on counts and offsets, where every member's outputs start, which draw a (member, slot) carries in pass k,
// the slots (NV) of a pass and the number of passes.  score_samples_batch.hpp drives the device by it;
// tests/tools/samples_batch_plan_check.cpp walks it against tables written by hand, stand-alone under the host sanitizers.
//
// Pass k of width W solves draw first_sample + k W + c of EVERY member in slot c; a member with S_g <= k W has dropped out.
// NV of a pass is the smallest of 1, 2, 4, 8, 16 that holds the most live slots of any member (gbs_slots: what mv_slots of
// score_marginals.hpp gives the marginals of a group).
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace score {

constexpr int kGbsMaxWidth = 16;  // slots of a pass at the most (kMvMaxWidth of score_marginals.hpp)

// what the plan needs of a member: its unknowns, the rows of one draw's noise, its packed moments, its selected unknowns
struct GbsShape {
    int64_t n, rows, moments, C;
};

inline int gbs_slots(int most) { return most <= 1 ? 1 : most <= 2 ? 2 : most <= 4 ? 4 : most <= 8 ? 8 : 16; }

struct GbsPlan {
    int G = 0, W = 0, passes = 0, most = 0;   // members, width, passes, the largest S_g
    int64_t first_sample = 0, samples = 0;    // samples: the sum of S_g
    std::vector<int32_t> count;               // [g] S_g
    std::vector<int32_t> cnt_ptr, probe_ptr;  // [g + 1] prefix sums of S_g, and of (S_g > 0): what the device reads
    // where member g starts in the outputs (G + 1 entries each; the last one is the output's size)
    std::vector<int64_t> draw_off, moments_off, means_off, steps_off, rhs_off, noise_off;

    // live slots of member g in pass k
    int live(int g, int k) const { return std::max(0, std::min(W, (int)count[(size_t)g] - k * W)); }
    // the member-local number of the draw in slot c of member g in pass k (-1: the slot carries none) ...
    int local_draw(int g, int c, int k) const { return c >= 0 && c < live(g, k) ? k * W + c : -1; }
    // ... and its index in the member's noise stream
    int64_t draw(int g, int c, int k) const {
        const int l = local_draw(g, c, k);
        return l < 0 ? -1 : first_sample + l;
    }
    // slots of pass k
    int nv(int k) const {
        int top = 0;
        for (int g = 0; g < G; ++g) top = std::max(top, live(g, k));
        return gbs_slots(top);
    }
};

// The checks on counts and offsets: what can be said without the graphs.  who: the entry point's name with ": ".
inline void gbs_check(const std::string& who, int G, const int32_t* n_samples, const uint64_t* seeds, const int32_t* var_ptr,
                      int64_t first_sample, int32_t block_width) {
    if (G < 1) throw std::runtime_error(who + "no members");
    if (!seeds) throw std::runtime_error(who + "seeds is null");
    if (!n_samples) throw std::runtime_error(who + "n_samples is null");
    if (!var_ptr) throw std::runtime_error(who + "var_ptr is null");
    if (block_width < 1 || block_width > kGbsMaxWidth) throw std::runtime_error(who + "block_width must be 1..16");
    if (var_ptr[0] != 0) throw std::runtime_error(who + "var_ptr must start at 0");
    int32_t most = 0;
    for (int g = 0; g < G; ++g) {
        if (var_ptr[g + 1] < var_ptr[g]) throw std::runtime_error(who + "var_ptr must not decrease");
        if (n_samples[g] < 0) throw std::runtime_error(who + "member " + std::to_string(g) + ": n_samples is negative");
        most = std::max(most, n_samples[g]);
    }
    if (most == 0) throw std::runtime_error(who + "n_samples is zero for every member");
    if (first_sample < 0 || first_sample + (int64_t)most > ((int64_t)1 << 32))
        throw std::runtime_error(who + "first_sample: draw indices must lie in 0 .. 2^32 - 1");
}

// The plan of a checked call.  shapes: one per member (C: the scalar unknowns of its selected variables).
inline GbsPlan gbs_plan(int G, const int32_t* n_samples, int64_t first_sample, int32_t block_width, const std::vector<GbsShape>& shapes) {
    GbsPlan p;
    p.G = G; p.W = block_width; p.first_sample = first_sample;
    p.count.assign(n_samples, n_samples + G);
    p.cnt_ptr.assign(1, 0); p.probe_ptr.assign(1, 0);
    for (std::vector<int64_t>* v : {&p.draw_off, &p.moments_off, &p.means_off, &p.steps_off, &p.rhs_off, &p.noise_off}) v->assign(1, 0);
    for (int g = 0; g < G; ++g) {
        const int64_t S = n_samples[g];
        const GbsShape& s = shapes[(size_t)g];
        p.most = std::max(p.most, (int)S);
        if (p.cnt_ptr.back() > INT32_MAX - S) throw std::runtime_error("score_refine_batch_samples: too many draws for one call");
        p.cnt_ptr.push_back((int32_t)(p.cnt_ptr.back() + S));
        p.probe_ptr.push_back(p.probe_ptr.back() + (S > 0 ? 1 : 0));
        p.draw_off.push_back(p.draw_off.back() + S);
        // (a member that takes no part has no room in the outputs)
        p.moments_off.push_back(p.moments_off.back() + (S > 0 ? s.moments : 0));
        p.means_off.push_back(p.means_off.back() + (S > 0 ? s.n : 0));
        p.steps_off.push_back(p.steps_off.back() + S * s.C);
        p.rhs_off.push_back(p.rhs_off.back() + S * s.n);
        p.noise_off.push_back(p.noise_off.back() + S * s.rows);
    }
    p.samples = p.draw_off.back();
    p.passes = (p.most + p.W - 1) / p.W;
    return p;
}

}  // namespace score

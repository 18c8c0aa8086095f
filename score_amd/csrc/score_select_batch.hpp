// score_select_batch.hpp -- greedy selection of candidate ranges for every member of a refinement group
// (include/score_select_batch.h): the selection of score_select.hpp crossed with the group's range
// variances (score_leverage_batch.hpp, section 21).
//
// What exists already and is used as it is: the columns of gbl_pair_solve, which takes the consumer of a solved pass defined
// here (GbSelCross) the way gbs_solve takes GblMeasure; lv_pair_dot_lane on the member's gb_view (a diagonal entry of P_g is
// the variance of k_gbl_pair_dot bit for bit); the bodies of score_select.hpp (sel_sym_tile_pair, sel_greedy_workgroup: what
// k_sel_sym / k_sel_greedy call on one graph) and the rule they decide by (score_select_rule.hpp).  The plan -- where a
// member's P, L and picks start, the workgroup -> (member, tile pair) table, the members with candidates -- is
// score_select_batch_plan.hpp's (HIP-free).  New here:
//   k_gbsel_cross<DIM>  after each pass, grid (ceil(pairs / kThreads), live slots): one lane per listed pair of the whole
//                       group, whatever its member; the lane of candidate c of member g writes
//                       P_g[c C_g + k W + s] = g_c'x_{g,s} for s < live(g, k); a lane whose member has dropped out returns
//   k_gbsel_sym         A_g = I + D_g (P_g + P_g')/2 D_g in place for every member in ONE launch, one workgroup per
//                       (member, tile pair); per-workgroup partials of max |P_cd - P_dc|, folded by the host per member in
//                       workgroup order
//   k_gbsel_greedy      ONE launch, one workgroup of kThreads lanes per member with candidates: the whole pivoted
//                       factorisation of that member (LDS per workgroup as k_sel_greedy's, under 40 KB: a CU holds it)
// fp64, no atomics, fixed-order sums; every workgroup belongs to one member or finds its lane's member from a table, so a
// member's numbers are those of a group that holds it alone.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/score_select_batch.h"
#include "score_leverage_batch.hpp"
#include "score_select.hpp"
#include "score_select_batch_plan.hpp"

namespace score {

static_assert(kGbSelTile == kSelTile, "the plan's tile is the transpose's");

struct GbSelArgs {
    const int32_t* pair_ptr;      // [g + 1]
    const int32_t* pair_member;   // [pair]
    const int32_t* pa; const int32_t* pb;
    int n_pairs;
    const int64_t* mat0;          // [g] member g's block of P
    const int64_t* l0;            // [g] ... of L
    const int32_t* pick0;         // [g] ... of order, gains, pick_var
    const int32_t* k;             // [g]
    const GbSelTilePair* tile;    // [workgroup of k_gbsel_sym]
    const int32_t* active;        // [workgroup of k_gbsel_greedy] its member
    double* P; double* L;
    const double* w;              // [pair] precisions
    const int32_t* excluded;      // [pair]
    double min_gain;
    int32_t* order; double* gains; double* pick_var;   // [pick0[g] + j]
    double* remaining;            // [pair]
    int32_t* picked;              // [g]
    double* part;                 // [workgroup of k_gbsel_sym]
};

// grid (ceil(pairs / kThreads), live slots of the pass): lane = listed pair, blockIdx.y = slot
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gbsel_cross(GbsArgs a, GbSelArgs e, const double* __restrict__ x) {
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= e.n_pairs) return;
    const int g = e.pair_member[p], s = blockIdx.y;
    if (s >= gbs_live(a, g)) return;
    const GbMember M = a.d.members[g];
    const int first = e.pair_ptr[g], C = e.pair_ptr[g + 1] - first, c = (int)p - first;
    double rho;
    lv_pair_dot_lane<DIM>(gb_view<DIM>(a.d, M, a.X, nullptr, nullptr), e.pa[p], e.pb[p], x + M.col0, a.n, s,
                          e.P + e.mat0[g] + (size_t)c * C + a.k0 + s, &rho);
}

// one workgroup per (member, tile pair)
__global__ __launch_bounds__(kThreads) void k_gbsel_sym(GbSelArgs e) {
    const GbSelTilePair t = e.tile[blockIdx.x];
    const int first = e.pair_ptr[t.member];
    sel_sym_tile_pair(e.P + e.mat0[t.member], e.w + first, e.pair_ptr[t.member + 1] - first, t.i, t.j, e.part + blockIdx.x);
}

// one workgroup per member with candidates
__global__ __launch_bounds__(kThreads) void k_gbsel_greedy(GbSelArgs e) {
    const int g = e.active[blockIdx.x], first = e.pair_ptr[g];
    SelGreedyArgs a;
    a.A = e.P + e.mat0[g]; a.w = e.w + first; a.excluded = e.excluded + first; a.C = e.pair_ptr[g + 1] - first; a.k = e.k[g];
    a.min_gain = e.min_gain; a.L = e.L + e.l0[g];
    a.order = e.order + e.pick0[g]; a.gains = e.gains + e.pick0[g]; a.pick_var = e.pick_var + e.pick0[g];
    a.remaining = e.remaining + first; a.picked = e.picked + g;
    sel_greedy_workgroup(a);
}

// The buffers of the call: device allocations of their own (not the handle's arena); they come with the first call, grow on
// demand and go with the handle, like GblWork.
struct GbSelWork {
    DevBuf<double> P, L, w, remaining, gains, pick_var, part;
    DevBuf<int32_t> excluded, order, picked, pick0, k, active;
    DevBuf<int64_t> mat0, l0;
    DevBuf<GbSelTilePair> tile;
    size_t p_room = 0, l_room = 0, pair_room = 0, pick_room = 0, tile_room = 0, g_room = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void reserve(const GbSelPlan& plan, hipStream_t st) {
        NoArena no_arena;
        const size_t G = (size_t)plan.G, pairs = (size_t)plan.pairs, picks = (size_t)plan.picks, tiles = plan.tile.size();
        const bool grows = (size_t)plan.entries > p_room || (size_t)plan.l_entries > l_room || pairs > pair_room || picks > pick_room ||
                           tiles > tile_room || G > g_room || !P.d;
        if (!grows) return;
        HIP_CHECK(sync_stream(st));  // (nothing queued still reads the buffers that go)
        if ((size_t)plan.entries > p_room || !P.d) { p_room = (size_t)plan.entries; P.alloc(p_room); }
        if ((size_t)plan.l_entries > l_room || !L.d) { l_room = (size_t)plan.l_entries; L.alloc(l_room); }
        if (pairs > pair_room || !w.d) { pair_room = pairs; w.alloc(pairs); remaining.alloc(pairs); excluded.alloc(pairs); }
        if (picks > pick_room || !order.d) { pick_room = picks; order.alloc(picks); gains.alloc(picks); pick_var.alloc(picks); }
        if (tiles > tile_room || !tile.d) { tile_room = tiles; tile.alloc(tiles); part.alloc(tiles); }
        if (G > g_room || !mat0.d) { g_room = G; mat0.alloc(G); l0.alloc(G); pick0.alloc(G); k.alloc(G); active.alloc(G); picked.alloc(G); }
    }
    ~GbSelWork() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

struct GbSelOutputs {
    int32_t* order; double* gains; double* pick_variances; double* remaining; int32_t* picked; double* total_gains;
};

// What score_refine_batch_select_ranges does with a solved pass of gbl_pair_solve, and with all of them.
struct GbSelCross {
    const double* precisions; const int32_t* k; double min_gain;
    GbSelOutputs out; double* matrix; score_select_batch_info* info;
    GbSelPlan plan;
    GbSelWork* W = nullptr;
    GbSelArgs e{};
    int dim = 2;
    bool pending = false;
    double cross_ms = 0.0;
    void settle() {   // (the pass's own read of its residuals has waited for the stream)
        if (!pending) return;
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, W->ev0, W->ev1));
        cross_ms += ms;
        pending = false;
    }
    void check(const GblPlan& pairs, const std::string& who) { plan = gbsel_plan(who, pairs.G, pairs.pair_ptr, precisions, k, min_gain); }
    void nothing(const GblPlan& pairs) {
        for (int g = 0; g < pairs.G; ++g) {
            if (out.picked) out.picked[g] = 0;
            if (out.total_gains) out.total_gains[g] = 0.0;
        }
        if (info) {
            const score_marginals_batch_info solve = info->solve;
            *info = score_select_batch_info{};
            info->solve = solve; info->members = pairs.G;
        }
    }
    template <class Batch>
    void begin(Batch& B, const GblPlan& pairs, const GbsArgs&, const GblArgs& l, hipStream_t st) {
        W = &B.gbsel;
        dim = B.U.dim;
        W->reserve(plan, st);
        if (!W->ev0) { HIP_CHECK(hipEventCreate(&W->ev0)); HIP_CHECK(hipEventCreate(&W->ev1)); }
        const size_t G = (size_t)plan.G;
        staged_h2d(W->w.d, precisions, (size_t)plan.pairs * sizeof(double), st);
        staged_h2d(W->mat0.d, plan.mat0.data(), G * sizeof(int64_t), st);
        staged_h2d(W->l0.d, plan.l0.data(), G * sizeof(int64_t), st);
        staged_h2d(W->pick0.d, plan.pick0.data(), G * sizeof(int32_t), st);
        staged_h2d(W->k.d, plan.k.data(), G * sizeof(int32_t), st);
        staged_h2d(W->active.d, plan.active.data(), plan.active.size() * sizeof(int32_t), st);
        staged_h2d(W->tile.d, plan.tile.data(), plan.tile.size() * sizeof(GbSelTilePair), st);
        e.pair_ptr = B.gbl.pair_ptr.d; e.pair_member = l.pair_member; e.pa = l.pa; e.pb = l.pb; e.n_pairs = (int)pairs.pairs;
        e.mat0 = W->mat0.d; e.l0 = W->l0.d; e.pick0 = W->pick0.d; e.k = W->k.d; e.tile = W->tile.d; e.active = W->active.d;
        e.P = W->P.d; e.L = W->L.d; e.w = W->w.d; e.excluded = W->excluded.d; e.min_gain = min_gain;
        e.order = W->order.d; e.gains = W->gains.d; e.pick_var = W->pick_var.d; e.remaining = W->remaining.d; e.picked = W->picked.d;
        e.part = W->part.d;
    }
    template <class Batch>
    void pass(Batch&, const GblPlan& pairs, const GbsArgs& q, int k_pass, const double* x, hipStream_t st) {
        settle();
        int live = 0;
        for (int g = 0; g < pairs.G; ++g) live = std::max(live, pairs.live(g, k_pass));
        if (live == 0) return;
        HIP_CHECK(hipEventRecord(W->ev0, st));
        gn_dim(dim, [&](auto d) {
            hipLaunchKernelGGL(k_gbsel_cross<decltype(d)::value>, dim3((unsigned)((pairs.pairs + kThreads - 1) / kThreads), (unsigned)live),
                               dim3(kThreads), 0, st, q, e, x);
        });
        HIP_CHECK(hipEventRecord(W->ev1, st));
        pending = true;
    }
    // col_done: 1 where the pair's column converged; the others' candidates are excluded in their members
    void end(const GblPlan& pairs, const std::vector<int32_t>& col_done, hipStream_t st) {
        settle();
        const double t0 = now_ms();
        const size_t C = (size_t)plan.pairs, G = (size_t)plan.G, picks = (size_t)plan.picks, tiles = plan.tile.size();
        if (matrix) staged_d2h(matrix, W->P.d, (size_t)plan.entries * sizeof(double), st);
        std::vector<int32_t> excluded(C);
        int32_t n_excluded = 0;
        for (size_t c = 0; c < C; ++c) n_excluded += excluded[c] = col_done[c] ? 0 : 1;
        staged_h2d(W->excluded.d, excluded.data(), C * sizeof(int32_t), st);
        hipLaunchKernelGGL(k_gbsel_sym, dim3((unsigned)tiles), dim3(kThreads), 0, st, e);
        hipLaunchKernelGGL(k_gbsel_greedy, dim3((unsigned)plan.active.size()), dim3(kThreads), 0, st, e);
        HIP_CHECK(hipGetLastError());
        std::vector<double> part(tiles), gains(picks);
        std::vector<int32_t> picked(G, 0);
        staged_d2h(part.data(), W->part.d, tiles * sizeof(double), st);
        staged_d2h(gains.data(), W->gains.d, picks * sizeof(double), st);
        staged_d2h(picked.data(), W->picked.d, G * sizeof(int32_t), st);
        if (out.order) staged_d2h(out.order, W->order.d, picks * sizeof(int32_t), st);
        if (out.pick_variances) staged_d2h(out.pick_variances, W->pick_var.d, picks * sizeof(double), st);
        if (out.remaining) staged_d2h(out.remaining, W->remaining.d, C * sizeof(double), st);
        HIP_CHECK(sync_stream(st));
        double worst = 0.0, total = 0.0;
        int32_t all_picked = 0;
        for (int g = 0; g < plan.G; ++g) {
            if (plan.count[(size_t)g] == 0) picked[(size_t)g] = 0;   // (no workgroup wrote it)
            double asym = 0.0, sum = 0.0;   // the member's partials in workgroup order, its gains in the order of the picks
            for (int32_t b = plan.wg0[(size_t)g]; b < plan.wg0[(size_t)g + 1]; ++b)
                if (part[(size_t)b] > asym) asym = part[(size_t)b];
            for (int32_t j = 0; j < picked[(size_t)g]; ++j) sum += gains[(size_t)plan.pick0[(size_t)g] + (size_t)j];
            if (asym > worst) worst = asym;
            total += sum;
            all_picked += picked[(size_t)g];
            if (out.picked) out.picked[g] = picked[(size_t)g];
            if (out.total_gains) out.total_gains[g] = sum;
        }
        if (out.gains) std::copy(gains.begin(), gains.end(), out.gains);
        if (info) {
            info->members = plan.G; info->candidates = (int32_t)plan.pairs; info->picked = all_picked; info->excluded = n_excluded;
            info->total_gain = total; info->asymmetry = worst; info->cross_ms = cross_ms; info->greedy_ms = now_ms() - t0;
        }
        (void)pairs;
    }
};

}  // namespace score

// score_leverage_batch.hpp -- leverage of the measurements and predicted range variances of every member of a refinement
// group (include/score_leverage_batch.h): the per-measurement sums of score_leverage.hpp crossed with
// the group's draws (score_samples_batch.hpp, section 18) and the group's gated iteration (score_group_pcg.hpp, section 12).
//
// What exists already and is used as it is: the draws (gbs_solve: noise, J'z, the probe per member, the passes, the
// verdicts, the per-member take masks), the lane bodies of score_leverage.hpp (lv_measure_lane, lv_pair_lane, lv_pair_entry,
// lv_pair_dot_lane: what k_lv_measure / k_lv_pair_rhs / k_lv_pair_dot call on one graph) on the member's gb_view<DIM>,
// group_pcg with a right-hand-side callback, gbm_product and k_gbs_residual (with cnt_ptr = pair_ptr) for the true
// residuals, GbmWork for the iteration's vectors and GbsWork::b for the right-hand sides -- no second copy of either --,
// mv_report.  The plan -- where a member's sums and pairs start, a pair's member, pass and slot -- is
// score_leverage_batch_plan.hpp's (HIP-free).  New here:
//   k_gbl_measure<DIM>   grid over mblk_member, one lane per measurement of the workgroup's member: lv_measure_lane with the
//                        member's seed, live slots and take mask; the four running sums at [k * M + meas0[g] + m], M the
//                        group's measurements (consecutive lanes, consecutive entries)
//   k_gbl_pairs<DIM>     one lane per listed pair of the whole group, its member from pair_member: lv_pair_lane (a workgroup
//                        may straddle members; every lane takes live / take from its own)
//   k_gbl_pair_rhs<DIM>  grid (unknown workgroups, NV): x = 0, r = b = g of the slot's pair; a slot beyond the member's pairs
//                        gets r = 0 and done word 1
//   k_gbl_pair_dot<DIM>  one lane per (member, slot) that carries a pair: lv_pair_dot_lane
// No atomics; every sum has a fixed order; every workgroup belongs to one member or finds its lane's member from a table,
// reads that member's live-slot count first and returns where it is zero, so a member's numbers are those of a group that
// holds it alone.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/score_leverage_batch.h"
#include "score_leverage.hpp"
#include "score_leverage_batch_plan.hpp"
#include "score_samples_batch.hpp"

namespace score {

struct GblArgs {
    double* sums;                 // [k * stride + meas0[g] + m], k = 0..3: the running sums of t, t^2, v, v^2
    long long stride;             // the measurements of the whole group
    const int64_t* meas0;         // [g]
    const int32_t* pair_member;   // [pair]
    const int32_t* pa; const int32_t* pb;
    int n_pairs;
    double* pair_sums;            // [k * n_pairs + pair], k = 0..1
    double* var; double* dist;    // [pair]
};

// one measurement of the workgroup's member per lane (lv_measure_lane on the member's view)
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gbl_measure(GbsArgs a, GblArgs l, const double* __restrict__ x) {
    const int g = a.d.mblk_member[blockIdx.x];
    const int live = gbs_live(a, g);
    if (live == 0) return;
    const unsigned take = a.take[g];
    if (take == 0u) return;
    const GbMember M = a.d.members[g];
    const long long m = (long long)((int)blockIdx.x - M.mblk0) * kThreads + threadIdx.x;
    lv_measure_lane<DIM>(gb_view<DIM>(a.d, M, a.X, nullptr, nullptr), m, x + M.col0, a.n, a.seeds[g], a.s0, live, take,
                         l.sums + l.meas0[g], l.stride);
}

// one listed pair per lane, whatever its member
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gbl_pairs(GbsArgs a, GblArgs l, const double* __restrict__ x) {
    const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= l.n_pairs) return;
    const int g = l.pair_member[p];
    const int live = gbs_live(a, g);
    if (live == 0) return;
    const unsigned take = a.take[g];
    if (take == 0u) return;
    const GbMember M = a.d.members[g];
    lv_pair_lane<DIM>(gb_view<DIM>(a.d, M, a.X, nullptr, nullptr), l.pa[p], l.pb[p], x + M.col0, a.n, live, take, l.pair_sums + p,
                      l.pair_sums + l.n_pairs + p);
}

// grid (unknown workgroups, NV): every thread owns one row of its member's column.  a.cnt_ptr is pair_ptr: slot c of member g
// carries its pair a.k0 + c.
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gbl_pair_rhs(GbmArgs p, GbsArgs a, GblArgs l) {
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y, t = threadIdx.x;
    const GbMember M = a.d.members[g];
    const bool on = c < gbs_live(a, g);
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + t;
    if (li < M.n) {
        const long long e = c * p.n + M.col0 + li;
        double gv = 0.0;
        if (on) {
            const long long pair = a.cnt_ptr[g] + a.k0 + c;
            gv = lv_pair_entry<DIM>(gb_view<DIM>(a.d, M, a.X, nullptr, nullptr), l.pa[pair], l.pb[pair], li);
        }
        p.x[e] = 0.0;
        p.r[e] = gv;
        a.b[e] = gv;
    }
    if ((int)blockIdx.x == M.ublk0 && t == 0) {
        p.done[g * p.NV + c] = on ? 0 : 1;
        p.iters[g * p.NV + c] = 0;
        p.ref[g * p.NV + c] = 0.0;
    }
}

// one lane per (member, slot) of the pass, slot-fastest; those that carry a pair: its variance and distance
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gbl_pair_dot(GbsArgs a, GblArgs l, const double* __restrict__ x, int G) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    const int g = t / a.width, c = t % a.width;
    if (g >= G || c >= gbs_live(a, g)) return;
    const GbMember M = a.d.members[g];
    const long long pair = a.cnt_ptr[g] + a.k0 + c;
    lv_pair_dot_lane<DIM>(gb_view<DIM>(a.d, M, a.X, nullptr, nullptr), l.pa[pair], l.pb[pair], x + M.col0, a.n, c, l.var + pair, l.dist + pair);
}

// The buffers of both calls: device allocations of their own (not the handle's arena); they come with the first call and go
// with the handle (the pairs' grow on demand).
struct GblWork {
    DevBuf<double> sums, pair_sums, var, dist;
    DevBuf<int64_t> meas0;
    DevBuf<int32_t> pa, pb, pair_member, pair_ptr;
    size_t pair_room = 0;
    void reserve(const GblPlan& plan, bool with_sums, hipStream_t st) {
        NoArena no_arena;
        if (with_sums && !sums.d) {
            sums.alloc(4 * (size_t)std::max<int64_t>(1, plan.meas));
            meas0.alloc((size_t)plan.G);
            staged_h2d(meas0.d, plan.meas0.data(), (size_t)plan.G * sizeof(int64_t), st);
        }
        if (!pair_ptr.d) pair_ptr.alloc((size_t)plan.G + 1);
        if ((size_t)plan.pairs > pair_room || !pa.d) {
            HIP_CHECK(sync_stream(st));  // (nothing queued still reads the buffers that go)
            pair_room = (size_t)std::max<int64_t>(16, plan.pairs);
            pa.alloc(pair_room); pb.alloc(pair_room); pair_member.alloc(pair_room);
            pair_sums.alloc(2 * pair_room); var.alloc(pair_room); dist.alloc(pair_room);
        }
    }
    void send_pairs(const GblPlan& plan, const int32_t* a, const int32_t* b, hipStream_t st) {
        staged_h2d(pair_ptr.d, plan.pair_ptr.data(), ((size_t)plan.G + 1) * sizeof(int32_t), st);
        if (plan.pairs == 0) return;
        const size_t bytes = (size_t)plan.pairs * sizeof(int32_t);
        staged_h2d(pa.d, a, bytes, st);
        staged_h2d(pb.d, b, bytes, st);
        staged_h2d(pair_member.d, plan.pair_member.data(), bytes, st);
    }
    GblArgs args(const GblPlan& plan) const {
        GblArgs l{};
        l.sums = sums.d; l.stride = plan.meas; l.meas0 = meas0.d; l.pair_member = pair_member.d; l.pa = pa.d; l.pb = pb.d;
        l.n_pairs = (int)plan.pairs; l.pair_sums = pair_sums.d; l.var = var.d; l.dist = dist.d;
        return l;
    }
};

inline std::vector<GblShape> gbl_shapes(const GbUnion& U) {
    std::vector<GblShape> shapes;
    for (const GbMember& M : U.members) shapes.push_back(GblShape{M.Np + M.Nl, M.n_rel + M.n_rng + M.n_pri});
    return shapes;
}

// What score_refine_batch_leverage does with a solved pass -- the consumer gbs_solve is given (as GbsMoments is the samples').
struct GblMeasure {
    const int32_t* pair_ptr; const int32_t* pair_a; const int32_t* pair_b;
    double* lev_sum; double* lev_sq; double* red_sum; double* red_sq; double* pair_sum; double* pair_sq;
    std::vector<int32_t> no_offsets;
    GblPlan plan;
    GblArgs l{};
    GblWork* L = nullptr;
    int dim = 2;
    // (the draws select no variables: offsets of zero)
    const int32_t* offsets(int G) {
        no_offsets.assign((size_t)std::max(G, 0) + 1, 0);
        return no_offsets.data();
    }
    void check(const GbUnion& U, const std::string& who, const int32_t* n_samples) {
        dim = U.dim;
        plan = gbl_plan(who, U.count, kGbsMaxWidth, n_samples, gbl_shapes(U), pair_ptr, pair_a, pair_b);
    }
    int64_t columns(int) const { return 0; }
    template <class Batch>
    void begin(Batch& B, GbsArgs&, const GbsPlan&, const std::vector<GbsShape>&, int, hipStream_t st) {
        L = &B.gbl;
        L->reserve(plan, true, st);
        L->send_pairs(plan, pair_a, pair_b, st);
        L->sums.zero(st); L->pair_sums.zero(st);
        l = L->args(plan);
    }
    template <class Batch>
    void pass(Batch& B, const GbsArgs& q, const GbsPass& p, hipStream_t st) {
        if (!p.any) return;
        const dim3 bt(kThreads);
        const unsigned pair_blocks = (unsigned)((plan.pairs + kThreads - 1) / kThreads);
        gn_dim(dim, [&](auto d) {
            hipLaunchKernelGGL(k_gbl_measure<decltype(d)::value>, dim3((unsigned)B.n_mblocks), bt, 0, st, q, l, p.x);
            if (pair_blocks) hipLaunchKernelGGL(k_gbl_pairs<decltype(d)::value>, dim3(pair_blocks), bt, 0, st, q, l, p.x);
        });
    }
    // the sums of the members that took part, member after member
    void end(const GbsPlan& draws, const std::vector<GbsShape>&, std::vector<double>& host, hipStream_t st) {
        double* out[4] = {lev_sum, lev_sq, red_sum, red_sq};
        if (out[0] || out[1] || out[2] || out[3]) {
            host.resize(4 * (size_t)plan.meas);
            staged_d2h(host.data(), L->sums.d, host.size() * sizeof(double), st);
            for (int k = 0; k < 4; ++k)
                for (int g = 0; out[k] && g < plan.G; ++g)
                    if (draws.count[(size_t)g] > 0) {
                        const double* from = host.data() + (size_t)k * (size_t)plan.meas + (size_t)plan.meas0[(size_t)g];
                        std::copy(from, from + (plan.meas_off[(size_t)g + 1] - plan.meas_off[(size_t)g]), out[k] + plan.meas_off[(size_t)g]);
                    }
        }
        const size_t np = (size_t)plan.pairs, f8 = sizeof(double);
        if (pair_sum && np) staged_d2h(pair_sum, L->pair_sums.d, np * f8, st);
        if (pair_sq && np) staged_d2h(pair_sq, L->pair_sums.d + np, np * f8, st);
    }
};

// What gbl_pair_solve does with a solved pass beyond its variances -- the consumer it is given, as gbs_solve is given
// GblMeasure and lv_pair_solve SelCross: check (the consumer's own arguments on the checked plan, before any work), nothing
// (nobody lists a pair: the call ends there), begin (the pairs are on the device, the arguments of the passes stand), pass
// (after k_gbl_pair_dot of pass k, its solutions still in x, column s at x + s n), end (every pass solved and read:
// col_done[pair] = 1 where the pair's column converged).  score_refine_batch_range_variances has none;
// score_refine_batch_select_ranges (score_select_batch.hpp) forms the members' cross terms.
struct GblPairOnly {
    void check(const GblPlan&, const std::string&) {}
    void nothing(const GblPlan&) {}
    template <class Batch>
    void begin(Batch&, const GblPlan&, const GbsArgs&, const GblArgs&, hipStream_t) {}
    template <class Batch>
    void pass(Batch&, const GblPlan&, const GbsArgs&, int, const double*, hipStream_t) {}
    void end(const GblPlan&, const std::vector<int32_t>&, hipStream_t) {}
};

// score_refine_batch_range_variances.  Batch: score_refine_batch (as gbm_solve; its GbsWork for the right-hand sides and its
// GblWork for the pairs).
template <class Batch, class Use>
int gbl_pair_solve(Batch& B, const std::string& who, const double* poses, const double* landmarks, const int32_t* pair_ptr,
                   const int32_t* pair_a, const int32_t* pair_b, double rel_tol, int32_t max_iters, int32_t block_width, double* variances,
                   double* distances, double* residuals, int32_t* iters, score_marginals_batch_info* info, Use& use) {
    const GbUnion& U = B.U;
    const int G = U.count, W = block_width;
    const GblPlan plan = gbl_plan(who, G, block_width, nullptr, gbl_shapes(U), pair_ptr, pair_a, pair_b);
    if (!(rel_tol > 0.0) || max_iters < 1) throw std::runtime_error(who + "rel_tol must be positive and max_iters >= 1");
    use.check(plan, who);
    if (plan.pairs == 0) {  // nothing listed: no device work
        if (info) *info = score_marginals_batch_info{};
        use.nothing(plan);
        return 0;
    }
    HipBackend& be = B.be();
    hipStream_t st = B.stream();
    const long long n = U.n;
    const double t0 = now_ms();
    // H of every member at its point, on the union pattern, lambda = 0; the chains of all members factored once: as gbm_solve
    B.set_point(poses, landmarks);
    B.eval(std::vector<char>((size_t)G, 1), false, true, nullptr);
    B.gather_h(std::vector<double>((size_t)G, 0.0).data());
    be.derive_rho_data(false);
    auto& K = B.mvb;
    auto& Q = B.gbs;
    auto& L = B.gbl;
    const size_t zb_per_vector = (size_t)be.H->bs * (size_t)be.n_join_seps;
    K.reserve(gbs_slots(std::min(W, plan.most)), (size_t)G, (size_t)n, (size_t)B.n_tiles, (size_t)B.n_ublocks, (size_t)be.n_prec, zb_per_vector, st);
    Q.reserve(B, gbs_shapes(U, [](int) { return 0; }), false, st);
    L.reserve(plan, false, st);
    L.send_pairs(plan, pair_a, pair_b, st);
    GbmArgs a = B.pcg_args();
    a.tol2 = rel_tol * rel_tol;
    a.res_part = K.res_part.d;
    a.sel_ptr = L.pair_ptr.d; a.width = W;
    GbsArgs q{};
    q.d = B.dev(); q.X = B.X.d; q.cnt_ptr = L.pair_ptr.d; q.width = W; q.b = Q.b.d; q.n = n;
    const GblArgs l = L.args(plan);
    use.begin(B, plan, q, l, st);
    const double t1 = now_ms();
    const dim3 bt(kThreads);
    const size_t nub = (size_t)B.n_ublocks, C = (size_t)plan.pairs;
    std::vector<int32_t> words, col_done(C, 0), col_iters(C, 0);
    std::vector<double> part, col_res(C, 0.0);
    int pcg_iters = 0;
    for (int k = 0; k < plan.passes; ++k) {
        const int NV = plan.nv(k);
        a.k0 = k * W;
        q.k0 = k * W;
        const dim3 gu((unsigned)B.n_ublocks, (unsigned)NV);
        group_pcg(be, a, K.pcg, NV, max_iters, K.zb.d, [&](const GbmArgs& p) {
            gn_dim(U.dim, [&](auto dim) { hipLaunchKernelGGL(k_gbl_pair_rhs<decltype(dim)::value>, gu, bt, 0, st, p, q, l); });
        }, words);
        // the true residual of every column of the pass (one more product, w = H x) against its g, and g'x
        a.all_slots = 1; a.p_in = K.pcg.x.d;
        gbm_product(a, st);
        hipLaunchKernelGGL(k_gbs_residual, gu, bt, 0, st, a, q, (const double*)a.w);
        const unsigned dot_blocks = (unsigned)((G * W + kThreads - 1) / kThreads);
        gn_dim(U.dim, [&](auto dim) {
            hipLaunchKernelGGL(k_gbl_pair_dot<decltype(dim)::value>, dim3(dot_blocks), bt, 0, st, q, l, (const double*)K.pcg.x.d, G);
        });
        use.pass(B, plan, q, k, (const double*)K.pcg.x.d, st);
        HIP_CHECK(hipGetLastError());
        part.resize((size_t)NV * nub);
        staged_d2h(part.data(), K.res_part.d, part.size() * sizeof(double), st);
        int most_steps = 0;
        for (int g = 0; g < G; ++g) {
            const GbMember& M = U.members[(size_t)g];
            for (int c = 0; c < plan.live(g, k); ++c) {
                double s = 0.0;  // the member's partials in workgroup order
                for (int blk = M.ublk0; blk < M.ublk1; ++blk) s += part[(size_t)c * nub + (size_t)blk];
                const double rho = std::sqrt(s);
                const size_t at = (size_t)plan.pair_at(g, c, k), word = (size_t)g * (size_t)NV + (size_t)c;
                col_res[at] = rho;
                col_done[at] = (words[word] == 1 && std::isfinite(rho)) ? 1 : 0;
                col_iters[at] = words[(size_t)G * (size_t)NV + word];
                most_steps = std::max(most_steps, col_iters[at]);
            }
        }
        pcg_iters += most_steps;
    }
    if (variances) staged_d2h(variances, L.var.d, C * sizeof(double), st);
    if (distances) staged_d2h(distances, L.dist.d, C * sizeof(double), st);
    HIP_CHECK(sync_stream(st));
    const double t2 = now_ms();
    double worst = 0.0;
    const int unconverged = mv_report(col_done, col_iters, col_res, residuals, iters, worst);
    if (info) {
        info->columns = (int32_t)plan.pairs; info->passes = plan.passes; info->pcg_iters = pcg_iters; info->unconverged = unconverged;
        info->max_residual = worst; info->setup_ms = t1 - t0; info->solve_ms = t2 - t1;
    }
    use.end(plan, col_done, st);
    return unconverged ? 1 : 0;
}

}  // namespace score

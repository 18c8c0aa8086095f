// score_relative_batch.hpp -- predicted relative poses between listed pairs of poses of every member of a refinement group
// and their covariances (include/score_relative_batch.h): the columns of score_relative.hpp on the
// group's gated iteration (score_group_pcg.hpp, section 12), driven as the ranges' group call is (gbl_pair_solve,
// score_leverage_batch.hpp).
//
// What exists already and is used as it is: the lane bodies of score_relative.hpp (rp_rhs_entry, rp_dot_lane: what k_rp_rhs /
// k_rp_dot call on one graph) on the member's gb_view<DIM>, group_pcg with a right-hand-side callback, gbm_product and
// k_gbs_residual (with cnt_ptr = col_ptr) for the true residuals, GbmWork for the iteration's vectors and GbsWork::b for the
// right-hand sides -- no second copy of either --, mv_report.  The plan -- the members' column offsets, a pair's member, the
// pair and error coordinate of a (member, slot, pass) -- is score_relative_batch_plan.hpp's (HIP-free).  New here:
//   k_grp_rhs<DIM>  grid (unknown workgroups, NV): a thread owns one row of its member's slot: x = 0, r = b = G_c'e_q of the
//                   slot's column; a slot beyond the member's columns gets zeros and done word 1; the member's first
//                   workgroup sets the done / iters / ref words
//   k_grp_dot<DIM>  one lane per (member, slot) of the pass, slot-fastest, those that carry a column: rp_dot_lane
// Neither uses LDS or atomics; every workgroup or lane reads its member's live-slot count first and returns where it is zero,
// and an output entry is formed from its own column alone in a fixed order: two calls give the same bits, and a member's
// numbers are those of a group that holds it alone.
//
// Access pattern.  k_grp_rhs is three coalesced n x NV streaming stores (consecutive lanes, consecutive rows of one member);
// only the at most 2 DP rows of a column's pair evaluate the Jacobian.  k_grp_dot reads 2 DP consecutive doubles twice per
// lane and stores DP entries DP apart: tens of bytes per column.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/score_relative_batch.h"
#include "score_relative.hpp"
#include "score_relative_batch_plan.hpp"
#include "score_samples_batch.hpp"

namespace score {

struct GrpArgs {
    const int32_t* pa; const int32_t* pb;     // [pair] member-local pose ids
    double* cov; double* rot; double* trans;  // per pair: DP x DP, DIM x DIM, DIM
};

// grid (unknown workgroups, NV): every thread owns one row of its member's slot.  a.cnt_ptr is col_ptr: slot c of member g
// carries its column a.k0 + c, global column col_ptr[g] + a.k0 + c -- pair / DP, error coordinate % DP.
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_grp_rhs(GbmArgs p, GbsArgs a, GrpArgs l) {
    constexpr int DP = DIM == 2 ? 3 : 6;
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y, t = threadIdx.x;
    const bool on = c < gbs_live(a, g);
    const GbMember M = a.d.members[g];
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + t;
    if (li < M.n) {
        const long long e = c * p.n + M.col0 + li;
        double gv = 0.0;
        if (on) {
            const long long j = (long long)a.cnt_ptr[g] + a.k0 + c, pair = j / DP;
            gv = rp_rhs_entry<DIM>(gb_view<DIM>(a.d, M, a.X, nullptr, nullptr), l.pa[pair], l.pb[pair], (int)(j - pair * DP), li);
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

// one lane per (member, slot) of the pass, slot-fastest; those that carry a column: its column of P, and with q == 0 the
// pair's R_ab and t_ab
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_grp_dot(GbsArgs a, GrpArgs l, const double* __restrict__ x, int G) {
    constexpr int DP = DIM == 2 ? 3 : 6;
    const int t = blockIdx.x * kThreads + threadIdx.x;
    const int g = t / a.width, c = t % a.width;
    if (g >= G || c >= gbs_live(a, g)) return;
    const GbMember M = a.d.members[g];
    const long long j = (long long)a.cnt_ptr[g] + a.k0 + c, pair = j / DP;
    const int q = (int)(j - pair * DP);
    rp_dot_lane<DIM>(gb_view<DIM>(a.d, M, a.X, nullptr, nullptr), l.pa[pair], l.pb[pair], q, x + M.col0, a.n, c,
                     l.cov + pair * (DP * DP) + q, l.rot + pair * (DIM * DIM), l.trans + pair * DIM);
}

// The buffers of the call: device allocations of their own (not the handle's arena); they come with the first call and go
// with the handle (the pairs' grow on demand).
struct GrpWork {
    DevBuf<double> cov, rot, trans;
    DevBuf<int32_t> pa, pb, pair_member, col_ptr;
    size_t pair_room = 0;
    void reserve(const GrpPlan& plan, int dim, hipStream_t st) {
        NoArena no_arena;
        if (!col_ptr.d) col_ptr.alloc((size_t)plan.G + 1);
        if ((size_t)plan.pairs > pair_room || !pa.d) {
            HIP_CHECK(sync_stream(st));  // (nothing queued still reads the buffers that go)
            const size_t dp = (size_t)plan.DP, d = (size_t)dim;
            pair_room = (size_t)std::max<int64_t>(16, plan.pairs);
            pa.alloc(pair_room); pb.alloc(pair_room); pair_member.alloc(pair_room);
            cov.alloc(pair_room * dp * dp); rot.alloc(pair_room * d * d); trans.alloc(pair_room * d);
        }
    }
    void send_pairs(const GrpPlan& plan, const int32_t* a, const int32_t* b, hipStream_t st) {
        staged_h2d(col_ptr.d, plan.col_ptr.data(), ((size_t)plan.G + 1) * sizeof(int32_t), st);
        const size_t bytes = (size_t)plan.pairs * sizeof(int32_t);
        staged_h2d(pa.d, a, bytes, st);
        staged_h2d(pb.d, b, bytes, st);
        staged_h2d(pair_member.d, plan.pair_member.data(), bytes, st);
    }
    GrpArgs args() const { return GrpArgs{pa.d, pb.d, cov.d, rot.d, trans.d}; }
};

// score_refine_batch_relative_covariances.  Batch: score_refine_batch (as gbl_pair_solve; its GbsWork for the right-hand
// sides and its GrpWork for the pairs).
template <class Batch>
int grp_solve(Batch& B, const double* poses, const double* landmarks, const int32_t* pair_ptr, const int32_t* pair_a,
              const int32_t* pair_b, double rel_tol, int32_t max_iters, int32_t block_width, double* rotations, double* translations,
              double* covariances, double* residuals, int32_t* iters, score_marginals_batch_info* info) {
    const GbUnion& U = B.U;
    const std::string who = "score_refine_batch_relative_covariances: ";
    const int G = U.count, W = block_width, DP = U.dp();
    std::vector<int64_t> n_poses;
    for (const GbMember& M : U.members) n_poses.push_back(M.Np);
    const GrpPlan plan = grp_plan(who, G, DP, block_width, n_poses, pair_ptr, pair_a, pair_b);
    if (!(rel_tol > 0.0) || max_iters < 1) throw std::runtime_error(who + "rel_tol must be positive and max_iters >= 1");
    if (plan.pairs == 0) {  // nothing listed: no device work
        if (info) *info = score_marginals_batch_info{};
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
    auto& L = B.grp;
    const size_t zb_per_vector = (size_t)be.H->bs * (size_t)be.n_join_seps;
    K.reserve(gbs_slots((int)std::min<int64_t>(W, plan.most)), (size_t)G, (size_t)n, (size_t)B.n_tiles, (size_t)B.n_ublocks, (size_t)be.n_prec,
              zb_per_vector, st);
    Q.reserve(B, gbs_shapes(U, [](int) { return 0; }), false, st);
    L.reserve(plan, U.dim, st);
    L.send_pairs(plan, pair_a, pair_b, st);
    GbmArgs a = B.pcg_args();
    a.tol2 = rel_tol * rel_tol;
    a.res_part = K.res_part.d;
    a.sel_ptr = L.col_ptr.d; a.width = W;
    GbsArgs q{};
    q.d = B.dev(); q.X = B.X.d; q.cnt_ptr = L.col_ptr.d; q.width = W; q.b = Q.b.d; q.n = n;
    const GrpArgs l = L.args();
    const double t1 = now_ms();
    const dim3 bt(kThreads);
    const size_t nub = (size_t)B.n_ublocks, C = (size_t)plan.columns;
    std::vector<int32_t> words, col_done(C, 0), col_iters(C, 0);
    std::vector<double> part, col_res(C, 0.0);
    int pcg_iters = 0;
    for (int k = 0; k < plan.passes; ++k) {
        const int NV = plan.nv(k);
        a.k0 = k * W;
        q.k0 = k * W;
        const dim3 gu((unsigned)B.n_ublocks, (unsigned)NV);
        group_pcg(be, a, K.pcg, NV, max_iters, K.zb.d, [&](const GbmArgs& p) {
            gn_dim(U.dim, [&](auto dim) { hipLaunchKernelGGL(k_grp_rhs<decltype(dim)::value>, gu, bt, 0, st, p, q, l); });
        }, words);
        // the true residual of every column of the pass (one more product, w = H x) against its right-hand side, and G x
        a.all_slots = 1; a.p_in = K.pcg.x.d;
        gbm_product(a, st);
        hipLaunchKernelGGL(k_gbs_residual, gu, bt, 0, st, a, q, (const double*)a.w);
        const unsigned dot_blocks = (unsigned)((G * W + kThreads - 1) / kThreads);
        gn_dim(U.dim, [&](auto dim) {
            hipLaunchKernelGGL(k_grp_dot<decltype(dim)::value>, dim3(dot_blocks), bt, 0, st, q, l, (const double*)K.pcg.x.d, G);
        });
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
                const GrpColumn col = plan.column_at(g, c, k);
                const size_t at = (size_t)col.pair * (size_t)DP + (size_t)col.q, word = (size_t)g * (size_t)NV + (size_t)c;
                col_res[at] = rho;
                col_done[at] = (words[word] == 1 && std::isfinite(rho)) ? 1 : 0;
                col_iters[at] = words[(size_t)G * (size_t)NV + word];
                most_steps = std::max(most_steps, col_iters[at]);
            }
        }
        pcg_iters += most_steps;
    }
    const size_t np = (size_t)plan.pairs, d = (size_t)U.dim, f8 = sizeof(double);
    if (covariances) staged_d2h(covariances, L.cov.d, np * (size_t)(DP * DP) * f8, st);
    if (rotations) staged_d2h(rotations, L.rot.d, np * d * d * f8, st);
    if (translations) staged_d2h(translations, L.trans.d, np * d * f8, st);
    HIP_CHECK(sync_stream(st));
    const double t2 = now_ms();
    double worst = 0.0;
    const int unconverged = mv_report(col_done, col_iters, col_res, residuals, iters, worst);
    if (info) {
        info->columns = (int32_t)plan.columns; info->passes = plan.passes; info->pcg_iters = pcg_iters; info->unconverged = unconverged;
        info->max_residual = worst; info->setup_ms = t1 - t0; info->solve_ms = t2 - t1;
    }
    return unconverged ? 1 : 0;
}

}  // namespace score

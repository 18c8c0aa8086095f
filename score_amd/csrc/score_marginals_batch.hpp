// score_marginals_batch.hpp -- marginal covariances of every member of a refinement group (include/score_marginals_batch.h):
// the block conjugate-gradient iteration of score_marginals.hpp crossed with the per-member control
// of score_gn_batch.hpp (section 12).
//
// The iteration itself -- NV union vectors advance NV columns of all members, every (member, slot) pair with its own alpha,
// beta, gate and done word -- is score_group_pcg.hpp's (group_pcg: kernels, buffers and the host loop), shared with the
// lock-step refinement.  What is the marginals' alone is here: in pass k of width W, slot c of member g carries that
// member's column k W + c; a slot with k W + c >= C_g gets r = 0 and done word 1 from the start (k_gbm_rhs).  NV is chosen per
// pass: the smallest of 1, 2, 4, 8, 16 that holds the most live slots of any member.  After the iteration of a pass: the true
// residual of every column from one more product w = H x (k_gbm_residual) and the selected rows of x (k_gbm_gather).
//
// What exists already and is used as it is: the blocks of all members (k_gb_blocks<DIM>), the gather of H on the union
// pattern (k_gb_gather_h, lambda = 0), one chain factorisation for all members (derive_rho_data -> k_factor), the verdict of
// a call from its columns (mv_report of score_marginals.hpp).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/score_marginals_batch.h"
#include "score_group_pcg.hpp"

namespace score {

// grid (unknown workgroups, NV): x = 0, r = the unit vector of the slot's unknown; the slot's words
__global__ __launch_bounds__(kThreads) void k_gbm_rhs(GbmArgs a) {
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y, t = threadIdx.x;
    const GbMember M = a.d.members[g];
    const int col = gbm_column(a, g, c);
    const long long unit = col >= 0 ? (long long)a.sel[a.sel_ptr[g] + col] : -1;
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + t;
    if (li < M.n) {
        const long long e = c * a.n + M.col0 + li;
        a.x[e] = 0.0;
        a.r[e] = li == unit ? 1.0 : 0.0;
    }
    if ((int)blockIdx.x == M.ublk0 && t == 0) {
        a.done[g * a.NV + c] = col >= 0 ? 0 : 1;
        a.iters[g * a.NV + c] = 0;
        a.ref[g * a.NV + c] = 0.0;
    }
}

// grid (unknown workgroups, NV): partials of |e_c - w_c|^2 with w = H x, on the slots that hold a column
__global__ __launch_bounds__(kThreads) void k_gbm_residual(GbmArgs a) {
    __shared__ double red[4];
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y, t = threadIdx.x;
    const int col = gbm_column(a, g, c);
    if (col < 0) return;
    const GbMember M = a.d.members[g];
    const long long unit = a.sel[a.sel_ptr[g] + col];
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + t;
    double dv = 0.0;
    if (li < M.n) dv = (li == unit ? 1.0 : 0.0) - a.w[c * a.n + M.col0 + li];
    const double s = block_sum(dv * dv, red);
    if (t == 0) a.res_part[(size_t)c * a.n_ublocks + blockIdx.x] = s;
}

// grid (blocks over all selected rows, NV): joint_g[s, k0 + c] = x_c[col0_g + sel_g[s]]
__global__ __launch_bounds__(kThreads) void k_gbm_gather(GbmArgs a) {
    const int c = blockIdx.y;
    const long long row = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (row >= a.n_sel) return;
    const int g = a.sel_member[row];
    const int col = gbm_column(a, g, c);
    if (col < 0) return;
    const long long Cg = a.sel_ptr[g + 1] - a.sel_ptr[g], s = row - a.sel_ptr[g];
    a.joint[a.joint_off[g] + s * Cg + col] = a.x[c * a.n + a.d.members[g].col0 + a.sel[row]];
}

// The selected unknowns of every member, member-local, in the order of include/score_marginals.h
inline void gbm_columns(const GbUnion& U, const int32_t* var_ptr, const int32_t* vars, std::vector<int32_t>& sel_ptr,
                        std::vector<int32_t>& sel) {
    if (!var_ptr) throw std::runtime_error("score_refine_batch_marginals: var_ptr is null");
    if (var_ptr[0] != 0) throw std::runtime_error("score_refine_batch_marginals: var_ptr must start at 0");
    sel_ptr.assign(1, 0);
    sel.clear();
    for (int g = 0; g < U.count; ++g) {
        const GbMember& M = U.members[(size_t)g];
        if (var_ptr[g + 1] < var_ptr[g]) throw std::runtime_error("score_refine_batch_marginals: var_ptr must not decrease");
        if (var_ptr[g + 1] > var_ptr[g] && !vars) throw std::runtime_error("score_refine_batch_marginals: vars is null");
        mv_variable_unknowns(M.Np, M.Nl, U.dp(), U.dim, vars + var_ptr[g], var_ptr[g + 1] - var_ptr[g],
                             "score_refine_batch_marginals: member " + std::to_string(g) + ": ", sel);
        if (sel.size() >= ((size_t)1 << 31)) throw std::runtime_error("score_refine_batch_marginals: too many columns");
        sel_ptr.push_back((int32_t)sel.size());
    }
}

// The block's buffers: device allocations of their own (not the handle's arena); they come with the first call, sized for
// the slots it needs, grow on demand and go with the handle.  At 64 worlds of 12 k unknowns a vector is 6 MB: 16 slots x 6
// buffers are about 0.6 GB.
struct GbmWork {
    GroupPcgWork pcg;
    DevBuf<double> res_part, zb;
    void reserve(int nv, size_t G, size_t n, size_t n_tiles, size_t n_ublocks, size_t n_prec, size_t zb_per_vector, hipStream_t st) {
        if (nv <= pcg.slots) return;
        NoArena no_arena;
        HIP_CHECK(sync_stream(st));  // (nothing queued still reads the buffers that go)
        if (!res_part.d) { res_part.alloc((size_t)kMvMaxWidth * n_ublocks); res_part.zero(st); }
        pcg.reserve(nv, kMvMaxWidth, G, n, n_tiles, n_ublocks, n_prec, st);
        zb.alloc((size_t)nv * std::max<size_t>(1, zb_per_vector)); zb.zero(st);
    }
};

// The solve.  Batch: score_refine_batch (its union, point, blocks and gather, its linear-mode handle, its GbmWork).
template <class Batch>
int gbm_solve(Batch& B, const double* poses, const double* landmarks, const int32_t* var_ptr, const int32_t* vars, double rel_tol,
              int32_t max_iters, int32_t block_width, double* joint, double* residuals, int32_t* iters, score_marginals_batch_info* info) {
    const GbUnion& U = B.U;
    if (block_width < 1 || block_width > kMvMaxWidth) throw std::runtime_error("score_refine_batch_marginals: block_width must be 1..16");
    if (!(rel_tol > 0.0) || max_iters < 1) throw std::runtime_error("score_refine_batch_marginals: rel_tol must be positive and max_iters >= 1");
    std::vector<int32_t> sel_ptr, sel;
    gbm_columns(U, var_ptr, vars, sel_ptr, sel);
    const int G = U.count, n_sel = (int)sel.size(), W = block_width;
    std::vector<long long> joint_off((size_t)G, 0);
    std::vector<int32_t> sel_member((size_t)n_sel, 0);
    size_t joint_size = 0;
    int most_columns = 0;
    for (int g = 0; g < G; ++g) {
        const size_t Cg = (size_t)(sel_ptr[(size_t)g + 1] - sel_ptr[(size_t)g]);
        joint_off[(size_t)g] = (long long)joint_size;
        joint_size += Cg * Cg;
        if (joint_size > ((size_t)1 << 27)) throw std::runtime_error("score_refine_batch_marginals: too many columns for one call (the C_g x C_g doubles beyond 1 GiB)");
        most_columns = std::max(most_columns, (int)Cg);
        std::fill(sel_member.begin() + sel_ptr[(size_t)g], sel_member.begin() + sel_ptr[(size_t)g + 1], g);
    }
    const int passes = (most_columns + W - 1) / W;
    HipBackend& be = B.be();
    hipStream_t st = B.stream();
    const long long n = U.n;
    const double t0 = now_ms();
    // H of every member at its point, on the union pattern, lambda = 0; the chains of all members factored once
    B.set_point(poses, landmarks);
    B.eval(std::vector<char>((size_t)G, 1), false, true, nullptr);
    B.gather_h(std::vector<double>((size_t)G, 0.0).data());
    be.derive_rho_data(false);
    std::vector<int32_t> col_done((size_t)n_sel, 0), col_iters((size_t)n_sel, 0);
    std::vector<double> col_res((size_t)n_sel, 0.0);
    int pcg_iters = 0;
    double t1 = now_ms();
    if (passes > 0) {
        auto& K = B.mvb;
        const size_t zb_per_vector = (size_t)be.H->bs * (size_t)be.n_join_seps;
        K.reserve(mv_slots(std::min(W, most_columns)), (size_t)G, (size_t)n, (size_t)B.n_tiles, (size_t)B.n_ublocks, (size_t)be.n_prec, zb_per_vector, st);
        DevBuf<int32_t> d_sel_ptr, d_sel, d_sel_member;
        DevBuf<long long> d_joint_off;
        DevBuf<double> d_joint;
        {
            NoArena no_arena;
            d_sel_ptr.alloc((size_t)G + 1); d_sel.alloc((size_t)n_sel); d_sel_member.alloc((size_t)n_sel);
            d_joint_off.alloc((size_t)G); d_joint.alloc(joint_size);
        }
        staged_h2d(d_sel_ptr.d, sel_ptr.data(), ((size_t)G + 1) * sizeof(int32_t), st);
        staged_h2d(d_sel.d, sel.data(), (size_t)n_sel * sizeof(int32_t), st);
        staged_h2d(d_sel_member.d, sel_member.data(), (size_t)n_sel * sizeof(int32_t), st);
        staged_h2d(d_joint_off.d, joint_off.data(), (size_t)G * sizeof(long long), st);
        GbmArgs a = B.pcg_args();
        a.tol2 = rel_tol * rel_tol;
        a.sel_ptr = d_sel_ptr.d; a.sel = d_sel.d; a.sel_member = d_sel_member.d; a.joint_off = d_joint_off.d; a.n_sel = n_sel;
        a.width = W; a.res_part = K.res_part.d; a.joint = d_joint.d;
        t1 = now_ms();
        const dim3 bt(kThreads);
        std::vector<int32_t> words;
        std::vector<double> res_part;
        for (int k = 0; k < passes; ++k) {
            int most = 0;
            for (int g = 0; g < G; ++g) most = std::max(most, std::min(W, sel_ptr[(size_t)g + 1] - sel_ptr[(size_t)g] - k * W));
            const int NV = mv_slots(most);
            a.k0 = k * W;
            const dim3 gu((unsigned)B.n_ublocks, (unsigned)NV);
            group_pcg(be, a, K.pcg, NV, max_iters, K.zb.d, [&](const GbmArgs& b) { hipLaunchKernelGGL(k_gbm_rhs, gu, bt, 0, st, b); }, words);
            // the true residual of every column of the pass (one more product, w = H x), the rows of S
            a.all_slots = 1; a.p_in = K.pcg.x.d;
            gbm_product(a, st);
            hipLaunchKernelGGL(k_gbm_residual, gu, bt, 0, st, a);
            hipLaunchKernelGGL(k_gbm_gather, dim3((unsigned)((n_sel + kThreads - 1) / kThreads), (unsigned)NV), bt, 0, st, a);
            HIP_CHECK(hipGetLastError());
            res_part.resize((size_t)NV * (size_t)B.n_ublocks);
            staged_d2h(res_part.data(), K.res_part.d, res_part.size() * sizeof(double), st);
            int most_steps = 0;
            for (int g = 0; g < G; ++g) {
                const GbMember& M = U.members[(size_t)g];
                const int Cg = sel_ptr[(size_t)g + 1] - sel_ptr[(size_t)g];
                for (int c = 0; c < W && k * W + c < Cg; ++c) {
                    double s = 0.0;  // the member's partials in workgroup order
                    for (int b = M.ublk0; b < M.ublk1; ++b) s += res_part[(size_t)c * (size_t)B.n_ublocks + (size_t)b];
                    const double rho = std::sqrt(s);
                    const size_t at = (size_t)sel_ptr[(size_t)g] + (size_t)(k * W + c), word = (size_t)g * (size_t)NV + (size_t)c;
                    col_res[at] = rho;
                    col_done[at] = (words[word] == 1 && std::isfinite(rho)) ? 1 : 0;
                    col_iters[at] = words[(size_t)G * (size_t)NV + word];
                    most_steps = std::max(most_steps, col_iters[at]);
                }
            }
            pcg_iters += most_steps;
        }
        if (joint && joint_size) staged_d2h(joint, d_joint.d, joint_size * sizeof(double), st);
        HIP_CHECK(sync_stream(st));
    }
    const double t2 = now_ms();
    double worst = 0.0;
    const int unconverged = mv_report(col_done, col_iters, col_res, residuals, iters, worst);
    if (info) {
        info->columns = n_sel; info->passes = passes; info->pcg_iters = pcg_iters; info->unconverged = unconverged;
        info->max_residual = worst; info->setup_ms = t1 - t0; info->solve_ms = t2 - t1;
    }
    return unconverged ? 1 : 0;
}

}  // namespace score

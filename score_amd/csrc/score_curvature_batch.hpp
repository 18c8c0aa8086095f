// score_curvature_batch.hpp -- the second-order check of EVERY member of a refinement group
// (include/score_curvature_batch.h): score_curvature.hpp crossed with score_spectrum_batch.hpp.
//
// E_g = J'J + sum_q r_q grad^2 r_q of member g lives on the member's part of the union pattern, so the group's iteration
// carries it as it is: gsp_iterate (one body, two operators) with GspArgs::val pointing at E_g + sigma_g I in a value array of
// this file's own, the Rayleigh-Ritz kernel with its `indefinite` word set, and the handle's GspWork.  The preconditioner
// stays that of J'J + sigma_g I, and the handle's K0 / Kset values stay J'J + sigma_g I: the Gauss-Newton quotients read them.
// The exact blocks go into block storage of their own, so the group's J'J blocks stand beside them for c_max_g.
//
// Every workgroup of every kernel belongs to one member, no reduction crosses a member boundary, there are no atomics, and
// the number and order of a member's partials depend on the member alone: a member's outputs are those of a group that holds
// it alone, and two calls give the same bits.  The per-lane bodies are score_curvature.hpp's (cv_blocks_lane,
// cv_gather_entry, cv_dot_terms), stated there once for a graph and a group.
//   k_gbc_blocks<DIM>   one measurement of the union per lane, laid over workgroups as k_gb_blocks lays them: its exact
//                       block (and its J'r again) into GbcWork's storage, through the member's gb_view
//   k_gbc_gather        one entry of the union pattern per lane: the sum of its exact (or J'J) slots in list order, + sigma_g
//                       on member g's diagonal, and the workgroup's maximum of |sum of exact slots - sum of J'J slots|.  The
//                       workgroups are cut from the members' entry ranges (GbcWork::gather_wgs), never across a member; the
//                       host joins a member's own workgroups to c_max_g
//   k_gbc_column_dots   grid (unknown workgroups, 16): the workgroup's partials of x_c'w_c and x_c'x_c
//   k_gbc_dots_sum      one workgroup per member: the partials of [ublk0, ublk1) summed in workgroup order
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/score_curvature_batch.h"
#include "score_curvature.hpp"
#include "score_spectrum_batch.hpp"

namespace score {

// grid (measurement workgroups)
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gbc_blocks(GbDev d, const double* __restrict__ X, double* __restrict__ eblk,
                                                         double* __restrict__ egblk) {
    const int g = d.mblk_member[blockIdx.x];
    const GbMember M = d.members[g];
    const long long m = (long long)((int)blockIdx.x - M.mblk0) * kThreads + threadIdx.x;
    cv_blocks_lane<DIM>(gb_view<DIM>(d, M, X, eblk, egblk), m);
}

struct GbcGatherArgs {
    const int32_t* hc_ptr; const int32_t* hc_slot;
    const double* hblk; const double* eblk;   // eblk null: J'J, no maxima asked
    const int32_t* diag_member;               // member + 1 on a diagonal entry, else 0
    const double* sigma;                      // [g]
    const int4* wgs;                          // {member, first entry, end entry, 0} per workgroup
    int exact;
    double* out; double* diff_part;
};

// grid (GbcWork::n_gather_wgs)
__global__ __launch_bounds__(kThreads) void k_gbc_gather(GbcGatherArgs a) {
    __shared__ double red[4];
    const int4 wg = a.wgs[blockIdx.x];
    const long long k = (long long)wg.y + threadIdx.x;
    double d = 0.0;
    if (k < wg.z) {
        const double v = cv_gather_entry(a.hc_ptr, a.hc_slot, a.hblk, a.eblk, a.exact, k, d);
        const int dm = a.diag_member[k];
        a.out[k] = dm ? v + a.sigma[dm - 1] : v;
    }
    d = block_max(d, red);
    if (threadIdx.x == 0) a.diff_part[blockIdx.x] = d;
}

// grid (unknown workgroups, 16): part[2 (c n_ublocks + workgroup)] = x_c'w_c, [.. + 1] = x_c'x_c over the workgroup's rows
__global__ __launch_bounds__(kThreads) void k_gbc_column_dots(GspArgs a, const double* __restrict__ w, double* __restrict__ part) {
    __shared__ double red[8];
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y;
    const GbMember M = a.d.members[g];
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + threadIdx.x;
    double xw = 0.0, xx = 0.0;
    if (li < M.n) {
        const long long e = c * a.n + M.col0 + li;
        cv_dot_terms(a.S[0][e], w[e], xw, xx);
    }
    block_sum2(xw, xx, red);
    if (threadIdx.x == 0) {
        const size_t at = 2 * ((size_t)c * (size_t)a.n_ublocks + blockIdx.x);
        part[at] = xw; part[at + 1] = xx;
    }
}

// grid (members), 64 lanes of which 32 work: dots[g][c][2], the member's partials in workgroup order
__global__ __launch_bounds__(64) void k_gbc_dots_sum(GspArgs a, const double* __restrict__ part, double* __restrict__ dots) {
    const int g = blockIdx.x, t = threadIdx.x;
    if (t >= 2 * kSpBlock) return;
    const GbMember M = a.d.members[g];
    const int c = t >> 1, which = t & 1;
    double acc = 0.0;
    for (int b = M.ublk0; b < M.ublk1; ++b) acc += part[2 * ((size_t)c * (size_t)a.n_ublocks + (size_t)b) + (size_t)which];
    dots[(size_t)g * (size_t)(2 * kSpBlock) + (size_t)t] = acc;
}

// The buffers of the group's curvature calls: device allocations of their own, they come with the first call and go with the
// handle.  The eight 16-vector blocks are the handle's GspWork.
struct GbcWork {
    DevBuf<double> val, eblk, egblk, diff_part, dot_part, dots;
    DevBuf<int4> gather_wgs;
    std::vector<int2> gather_range;  // [g] its workgroups [x, y) of the gather
    int n_gather_wgs = 0;
    template <class Batch>
    void reserve(Batch& B, hipStream_t st) {
        if (val.d) return;
        NoArena no_arena;
        const GbUnion& U = B.U;
        // the members' entry ranges, from the row pointers of the union pattern
        std::vector<int32_t> ptr((size_t)U.n + 1);
        staged_d2h(ptr.data(), B.be().Kset.mat.ptr.d, ptr.size() * sizeof(int32_t), st);
        HIP_CHECK(sync_stream(st));
        std::vector<int4> wgs;
        gather_range.clear();
        for (const GbMember& M : U.members) {
            const long long e0 = ptr[(size_t)M.col0], e1 = ptr[(size_t)(M.col0 + M.n)];
            const int first = (int)wgs.size();
            for (long long e = e0; e < e1; e += kThreads) wgs.push_back(make_int4((int)gather_range.size(), (int)e, (int)std::min<long long>(e + kThreads, e1), 0));
            gather_range.push_back(make_int2(first, (int)wgs.size()));
        }
        if (ptr[(size_t)U.n] != (int32_t)B.nnz) throw std::runtime_error("score_refine_batch_curvature: the union pattern and its row pointers disagree");
        n_gather_wgs = (int)wgs.size();
        gather_wgs.alloc(wgs.size()); staged_h2d(gather_wgs.d, wgs.data(), wgs.size() * sizeof(int4), st);
        val.alloc((size_t)B.nnz + 64); val.zero(st);  // (padded like the handle's own values)
        eblk.alloc((size_t)std::max<long long>(1, U.hblk_size)); eblk.zero(st);
        egblk.alloc((size_t)std::max<long long>(1, U.gblk_size)); egblk.zero(st);
        diff_part.alloc((size_t)std::max(1, n_gather_wgs)); diff_part.zero(st);
        dot_part.alloc((size_t)2 * kSpBlock * (size_t)B.n_ublocks); dot_part.zero(st);
        dots.alloc((size_t)2 * kSpBlock * (size_t)U.count); dots.zero(st);
    }
};

// The exact blocks at the members' current points (eval has run: the J'J blocks are in the handle's storage), then
// val = (exact ? E_g : J'J) + sigma_g I on the union pattern, sigma_g from the handle's `lambda`.  c_max (null: not asked):
// per member max |E_g - J'J| over its entries.
template <class Batch>
void gbc_values(Batch& B, bool exact, std::vector<double>* c_max) {
    hipStream_t st = B.stream();
    auto& C = B.gbc;
    C.reserve(B, st);
    if (exact)
        gn_dim(B.U.dim, [&](auto dim) {
            hipLaunchKernelGGL(k_gbc_blocks<decltype(dim)::value>, dim3((unsigned)B.n_mblocks), dim3(kThreads), 0, st, B.dev(),
                               (const double*)B.X.d, C.eblk.d, C.egblk.d);
        });
    GbcGatherArgs a{};
    a.hc_ptr = B.hc_ptr.d; a.hc_slot = B.hc_slot.d; a.hblk = B.hblk.d; a.eblk = exact ? C.eblk.d : nullptr;
    a.diag_member = B.diag_member.d; a.sigma = B.lambda.d; a.wgs = C.gather_wgs.d; a.exact = exact ? 1 : 0;
    a.out = C.val.d; a.diff_part = C.diff_part.d;
    hipLaunchKernelGGL(k_gbc_gather, dim3((unsigned)C.n_gather_wgs), dim3(kThreads), 0, st, a);
    HIP_CHECK(hipGetLastError());
    if (!c_max) return;
    std::vector<double> part((size_t)C.n_gather_wgs);
    staged_d2h(part.data(), C.diff_part.d, part.size() * sizeof(double), st);
    HIP_CHECK(sync_stream(st));
    c_max->assign((size_t)B.U.count, 0.0);
    for (int g = 0; g < B.U.count; ++g)
        for (int w = C.gather_range[(size_t)g].x; w < C.gather_range[(size_t)g].y; ++w)
            (*c_max)[(size_t)g] = std::max((*c_max)[(size_t)g], part[(size_t)w]);
}

// score_refine_batch_curvature's operator for gsp_iterate: A_g = E_g + sigma_g I from GbcWork::val, negative Ritz values
// allowed; after the rounds one more product of the final X with the Gauss-Newton values (the handle's: J'J + sigma_g I) into
// AW -- free once the rounds have ended -- and the members' column dots.
struct GspCurvature {
    static constexpr bool indefinite = true;
    const char* who = "score_refine_batch_curvature: ";
    std::vector<double> c_max;  // [g]
    std::vector<double> dots;   // [g][16][2]: x'w, x'x
    template <class Batch>
    const double* product_values(Batch& B) {
        gbc_values(B, true, &c_max);
        return B.gbc.val.d;
    }
    template <class Batch>
    void after_iteration(Batch& B, const GspArgs& a) {
        hipStream_t st = B.stream();
        auto& C = B.gbc;
        GspArgs gn = a;  // AW = (J'J + sigma_g I) X on all 16 columns of every member
        gn.val = B.be().Kset.mat.val.d; gn.AS[0] = a.AS[1]; gn.x_only = 1;
        hipLaunchKernelGGL(k_gsp_product, dim3((unsigned)a.n_tiles), dim3(kThreads), 0, st, gn);
        hipLaunchKernelGGL(k_gbc_column_dots, dim3((unsigned)a.n_ublocks, (unsigned)kSpBlock), dim3(kThreads), 0, st, a,
                           (const double*)a.AS[1], C.dot_part.d);
        hipLaunchKernelGGL(k_gbc_dots_sum, dim3((unsigned)B.U.count), dim3(64), 0, st, a, (const double*)C.dot_part.d, C.dots.d);
        HIP_CHECK(hipGetLastError());
        dots.resize((size_t)2 * kSpBlock * (size_t)B.U.count);
        staged_d2h(dots.data(), C.dots.d, dots.size() * sizeof(double), st);
    }
};

template <class Batch>
int gbc_solve(Batch& B, const double* poses, const double* landmarks, int32_t k, double rel_tol, int32_t max_iters, double shift_rel,
              double* values, double* vectors, double* residuals, double* gn_quotients, int32_t* iterations, double* h_max, double* c_max,
              score_curvature_batch_info* info) {
    GspCurvature op;
    GspOutcome o;
    const int rc = gsp_iterate(B, op, poses, landmarks, k, rel_tol, max_iters, shift_rel, values, vectors, residuals, iterations, h_max, o);
    HIP_CHECK(sync_stream(B.stream()));
    const int G = B.U.count;
    int saddles = 0;
    for (int g = 0; g < G; ++g) {
        bool negative = false;
        for (int j = 0; j < k; ++j) {
            const size_t at = (size_t)g * (size_t)k + (size_t)j;
            // pair j is column o.column[at] of X; the product read J'J + sigma_g I, and X is orthonormal only to rounding
            const double* d = op.dots.data() + ((size_t)g * kSpBlock + (size_t)o.column[at]) * 2;
            if (gn_quotients) gn_quotients[at] = d[0] / d[1] - o.sigma[(size_t)g];
            if (o.value[at] < -rel_tol * o.h_max[(size_t)g]) negative = true;
        }
        if (negative) ++saddles;
        if (c_max) c_max[g] = op.c_max[(size_t)g];
    }
    if (info) {
        info->members = G; info->modes = k; info->block = kSpBlock; info->rounds = o.rounds; info->unconverged = o.unconverged;
        info->saddles = saddles; info->max_residual = o.worst; info->setup_ms = o.setup_ms; info->solve_ms = o.solve_ms;
    }
    return rc;
}

// out_g = A_g V_g for every member in one launch over the union, A = E (exact) or J'J at the points, no shift.  V_g, out_g:
// n_cols x n_g row-major, the members one after the other.  Always the 16-column product over a zero-padded block: a column's
// sums do not depend on its neighbours, so fewer columns give the bits of the same columns at 16.
template <class Batch>
int gbc_product(Batch& B, const double* poses, const double* landmarks, int32_t exact, const double* V, int32_t n_cols, double* out) {
    const GbUnion& U = B.U;
    if (n_cols < 1 || n_cols > kSpBlock) throw std::runtime_error("score_refine_batch_hessian_product: n_cols must be 1..16");
    HipBackend& be = B.be();
    hipStream_t st = B.stream();
    const int G = U.count;
    const size_t n = (size_t)U.n, f8 = sizeof(double);
    auto& W = B.spb;
    W.reserve(U, (size_t)B.n_tiles, (size_t)B.n_ublocks, (size_t)be.n_prec, (size_t)be.H->bs * (size_t)be.n_join_seps, st);
    B.set_point(poses, landmarks);
    B.eval(std::vector<char>((size_t)G, 1), false, true, nullptr);
    const std::vector<double> no_shift((size_t)G, 0.0);
    staged_h2d(B.lambda.d, no_shift.data(), no_shift.size() * f8, st);
    gbc_values(B, exact != 0, nullptr);
    std::vector<double> block((size_t)kSpBlock * n, 0.0);  // column c of every member at c * n + col0_g
    size_t at = 0;
    for (const GbMember& M : U.members) {
        for (int c = 0; c < n_cols; ++c)
            std::copy(V + at + (size_t)c * (size_t)M.n, V + at + (size_t)(c + 1) * (size_t)M.n, block.begin() + (std::ptrdiff_t)((size_t)c * n + (size_t)M.col0));
        at += (size_t)n_cols * (size_t)M.n;
    }
    staged_h2d(W.x.d, block.data(), block.size() * f8, st);
    GspArgs a{};
    a.d = B.dev();
    a.ptr = be.Kset.mat.ptr.d; a.col = be.Kset.mat.col.d; a.val = B.gbc.val.d;
    a.tiles = B.tiles.d; a.n_tiles = B.n_tiles; a.n_ublocks = B.n_ublocks; a.n = U.n;
    a.S[0] = W.x.d; a.AS[0] = W.ax.d; a.ctl = W.ctl.d; a.flags = W.flags.d; a.pw_part = W.pw_part.d;
    a.x_only = 1;  // AX = A X on all 16 columns of every member
    hipLaunchKernelGGL(k_gsp_product, dim3((unsigned)B.n_tiles), dim3(kThreads), 0, st, a);
    HIP_CHECK(hipGetLastError());
    staged_d2h(block.data(), W.ax.d, (size_t)n_cols * n * f8, st);
    HIP_CHECK(sync_stream(st));
    at = 0;
    for (const GbMember& M : U.members) {
        for (int c = 0; c < n_cols; ++c) {
            const double* src = block.data() + (size_t)c * n + (size_t)M.col0;
            std::copy(src, src + M.n, out + at + (size_t)c * (size_t)M.n);
        }
        at += (size_t)n_cols * (size_t)M.n;
    }
    return 0;
}

}  // namespace score

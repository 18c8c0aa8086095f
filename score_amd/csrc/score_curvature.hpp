// score_curvature.hpp -- the second-order check of a refined estimate (include/score_curvature.h): half the Hessian of the
// cost, E = J'J + sum_q r_q grad^2 r_q (q over the whitened residual rows), on the device -- its product with a block of
// vectors and its lowest eigenpairs.
//
// E lives on the pattern of J'J: grad^2 r_q touches the unknowns of its own measurement only.  So everything that carries
// J'J carries E: the per-measurement block storage (gn_measurement<DIM, true> writes the exact block in the layout of the
// J'J block: score_gn.hpp, gn_rel_curv / gn_rel_curv3 / gn_range_curv), the contribution lists, the handle's pattern, the
// product k_mv_product<16> and the iteration of score_spectrum.hpp (sp_iterate: one body, two operators).  What does NOT
// carry over is the preconditioner: chain factors of an indefinite E need not exist, so M stays the chain part of
// J'J + sigma I, and the handle's own values and factors stay those of J'J + sigma I.  E + sigma I goes into a value array of
// this file's own (CvWork::val), which the product reads; the exact blocks go into block storage of their own, so the
// handle's J'J blocks stand beside them for the one figure that needs both: c_max = max |E_ij - (J'J)_ij| over the pattern.
//
// New kernels, one lane per item, streaming, like k_gn_blocks and k_gn_gather_h:
//   k_cv_blocks<DIM>  one measurement per lane: its exact block (and its J'r again) into CvWork's storage
//   k_cv_gather       one entry of the pattern per lane: the sum of its exact (or J'J) slots in list order, + sigma on the
//                     diagonal, and the workgroup's maximum of |sum of exact slots - sum of J'J slots| (host: the maximum of
//                     the workgroups, like k_sp_hmax)
//   k_cv_column_dots  one workgroup per column c: x_c'w_c and x_c'x_c, lanes stride the rows in ascending order, the
//                     workgroup's sum in the fixed order of block_sum2.  No atomics: two calls give the same bits.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/score_curvature.h"
#include "score_spectrum.hpp"

namespace score {

// The per-lane bodies, stated once for a graph (the kernels below) and for a group (score_curvature_batch.hpp):
//   cv_blocks_lane   measurement m of the view: its exact block and its J'r into the view's storage (a lane beyond the
//                    measurements: nothing)
//   cv_gather_entry  entry k of the pattern: the sum of its exact (or J'J) slots in list order, without the shift; diff =
//                    |sum of exact slots - sum of J'J slots| with a NaN counted as +inf (eblk == nullptr: not asked, zero)
//   cv_dot_terms     one row's terms of x'w and x'x
template <int DIM>
__device__ __forceinline__ void cv_blocks_lane(const GnView& v, int64_t m) {
    (void)gn_measurement<DIM, true>(v, m, true);
}
__device__ __forceinline__ double cv_gather_entry(const int32_t* __restrict__ hc_ptr, const int32_t* __restrict__ hc_slot,
                                                  const double* __restrict__ hblk, const double* __restrict__ eblk, int exact,
                                                  int64_t k, double& diff) {
    double h = 0.0, e = 0.0;
    for (int32_t c = hc_ptr[k]; c < hc_ptr[k + 1]; ++c) {
        const int32_t s = hc_slot[c];
        h += hblk[s];
        if (eblk) e += eblk[s];
    }
    diff = 0.0;
    if (eblk) {
        diff = fabs(e - h);
        diff = diff == diff ? diff : INFINITY;  // (fmax would drop a NaN)
    }
    return exact ? e : h;
}
__device__ __forceinline__ void cv_dot_terms(double xi, double wi, double& xw, double& xx) {
    xw += xi * wi;
    xx += xi * xi;
}

// one measurement of the view per lane
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_cv_blocks(GnView v) {
    cv_blocks_lane<DIM>(v, (int64_t)blockIdx.x * kThreads + threadIdx.x);
}

// one entry of the pattern per lane.  out = (exact ? sum of eblk slots : sum of hblk slots) (+ sigma on the diagonal);
// diff_part[workgroup] = max |sum of eblk slots - sum of hblk slots| (eblk == nullptr: not asked, zero)
__global__ __launch_bounds__(kThreads) void k_cv_gather(const int32_t* __restrict__ hc_ptr, const int32_t* __restrict__ hc_slot,
                                                        const double* __restrict__ hblk, const double* __restrict__ eblk,
                                                        const int32_t* __restrict__ is_diag, double sigma, int exact,
                                                        double* __restrict__ out, double* __restrict__ diff_part, int64_t nnz) {
    __shared__ double red[4];
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double d = 0.0;
    if (k < nnz) {
        const double v = cv_gather_entry(hc_ptr, hc_slot, hblk, eblk, exact, k, d);
        out[k] = is_diag[k] ? v + sigma : v;
    }
    d = block_max(d, red);
    if (threadIdx.x == 0) diff_part[blockIdx.x] = d;
}

// grid (columns): dots[2 c] = x_c'w_c, dots[2 c + 1] = x_c'x_c
__global__ __launch_bounds__(kThreads) void k_cv_column_dots(const double* __restrict__ x, const double* __restrict__ w, long long n,
                                                             double* __restrict__ dots) {
    __shared__ double red[8];
    const int c = blockIdx.x;
    const double* xc = x + (size_t)c * (size_t)n;
    const double* wc = w + (size_t)c * (size_t)n;
    double xw = 0.0, xx = 0.0;
    for (long long i = threadIdx.x; i < n; i += kThreads) {
        cv_dot_terms(xc[i], wc[i], xw, xx);
    }
    block_sum2(xw, xx, red);
    if (threadIdx.x == 0) { dots[2 * c] = xw; dots[2 * c + 1] = xx; }
}

// The buffers of the curvature calls: they stay with the refinement handle (device allocations of their own, as SpWork's).
struct CvWork {
    DevBuf<double> val, eblk, egblk, diff_part, dots;
    void reserve(const GnProblem& P, int n_hblocks, hipStream_t st) {
        if (val.d) return;
        NoArena no_arena;
        val.alloc(P.hcol.size() + 64); val.zero(st);  // (padded like the handle's own values)
        eblk.alloc((size_t)std::max<int64_t>(1, P.hblk_size())); eblk.zero(st);
        egblk.alloc((size_t)std::max<int64_t>(1, P.gblk_size())); egblk.zero(st);
        diff_part.alloc((size_t)std::max(1, n_hblocks)); diff_part.zero(st);
        dots.alloc((size_t)2 * kSpBlock); dots.zero(st);
    }
};

// The exact blocks at the handle's current point (h_at_point has run: the J'J blocks are in the handle's storage), then
// val = (exact ? E : J'J) + sigma I on the handle's pattern.  Returns c_max (exact) or 0.
template <class Refine>
double cv_values(Refine& R, bool exact, double sigma) {
    const GnProblem& P = R.P;
    hipStream_t st = R.stream();
    auto& C = R.cv;
    C.reserve(P, R.n_hblocks, st);
    if (exact) {
        GnView v = R.view(R.u.d);
        v.hblk = C.eblk.d; v.gblk = C.egblk.d;
        gn_dim(P.dim, [&](auto dim) { hipLaunchKernelGGL(k_cv_blocks<decltype(dim)::value>, dim3((unsigned)R.n_mblocks), dim3(kThreads), 0, st, v); });
    }
    hipLaunchKernelGGL(k_cv_gather, dim3((unsigned)R.n_hblocks), dim3(kThreads), 0, st, (const int32_t*)R.hc_ptr.d,
                       (const int32_t*)R.hc_slot.d, (const double*)R.hblk.d, exact ? (const double*)C.eblk.d : (const double*)nullptr,
                       (const int32_t*)R.is_diag.d, sigma, exact ? 1 : 0, C.val.d, C.diff_part.d, (int64_t)P.hcol.size());
    HIP_CHECK(hipGetLastError());
    if (!exact) return 0.0;
    std::vector<double> part((size_t)R.n_hblocks);
    staged_d2h(part.data(), C.diff_part.d, part.size() * sizeof(double), st);
    HIP_CHECK(sync_stream(st));
    double c_max = 0.0;
    for (double v : part) c_max = std::max(c_max, v);
    return c_max;
}

// score_refine_curvature's operator for sp_iterate: A = E + sigma I from CvWork::val, negative Ritz values allowed; after the
// iteration one more product of the final X with the Gauss-Newton values (the handle's: J'J + sigma I) and the column dots.
struct SpCurvature {
    static constexpr bool indefinite = true;
    const char* who = "score_refine_curvature: ";
    double c_max = 0.0;
    double dots[2 * kSpBlock] = {};
    template <class Refine>
    const double* product_values(Refine& R, double sigma) {
        c_max = cv_values(R, true, sigma);
        return R.cv.val.d;
    }
    template <class Refine, class Product>
    void after_iteration(Refine& R, Product& product_with, double) {
        auto& W = R.sp;
        product_with(R.be().Kset.mat.val.d, W.x.d, W.aw.d);  // (AW is free once the iteration has ended)
        hipLaunchKernelGGL(k_cv_column_dots, dim3((unsigned)kSpBlock), dim3(kThreads), 0, R.stream(), (const double*)W.x.d,
                           (const double*)W.aw.d, (long long)R.P.n, R.cv.dots.d);
        HIP_CHECK(hipGetLastError());
        staged_d2h(dots, R.cv.dots.d, sizeof(dots), R.stream());
    }
};

// out = A V with A = E (exact) or J'J at the point, no shift.  V, out: n_cols x n row-major, which is the block layout (column c
// at c * n).  Always the 16-column product over a zero-padded block: a column's sums do not depend on its neighbours, so
// fewer columns give the bits of the same columns at 16.
template <class Refine>
int cv_product(Refine& R, const double* poses, const double* landmarks, int32_t exact, const double* V, int32_t n_cols, double* out) {
    const GnProblem& P = R.P;
    if (n_cols < 1 || n_cols > kSpBlock) throw std::runtime_error("score_refine_hessian_product: n_cols must be 1..16");
    if (P.n < 1) throw std::runtime_error("score_refine_hessian_product: the graph has no unknowns");
    HipBackend& be = R.be();
    hipStream_t st = R.stream();
    const size_t n = (size_t)P.n, f8 = sizeof(double);
    R.h_at_point(poses, landmarks, "score_refine_hessian_product: ", nullptr);
    auto& W = R.sp;
    W.reserve(P, R.product_tiles(), be.n_prec, be.H->bs * be.n_join_seps, R.n_hblocks, st);
    (void)cv_values(R, exact != 0, 0.0);
    W.x.zero(st);
    staged_h2d(W.x.d, V, (size_t)n_cols * n * f8, st);
    MvArgs m{};
    m.ptr = be.Kset.mat.ptr.d; m.col = be.Kset.mat.col.d; m.val = R.cv.val.d;
    m.tiles = W.tiles; m.n_tiles = W.n_tiles; m.n = (long long)P.n; m.flags = W.flags.d; m.all_columns = 1; m.pw_part = W.pw_part.d;
    m.p_in = W.x.d; m.w = W.ax.d;
    hipLaunchKernelGGL(k_mv_product<kSpBlock>, dim3((unsigned)W.n_tiles), dim3(kMvThreads), 0, st, m);
    HIP_CHECK(hipGetLastError());
    staged_d2h(out, W.ax.d, (size_t)n_cols * n * f8, st);
    HIP_CHECK(sync_stream(st));
    return 0;
}

template <class Refine>
int cv_solve(Refine& R, const double* poses, const double* landmarks, int32_t k, double rel_tol, int32_t max_iters, double shift_rel,
             double* values, double* vectors, double* residuals, double* gn_quotients, score_curvature_info* info) {
    SpCurvature op;
    SpOutcome o;
    const int rc = sp_iterate(R, op, poses, landmarks, k, rel_tol, max_iters, shift_rel, values, vectors, residuals, o);
    // pair j is column o.column[j] of X; the product read J'J + sigma I, and X is orthonormal only to rounding
    if (gn_quotients)
        for (int j = 0; j < k; ++j) {
            const int c = o.column[j];
            gn_quotients[j] = op.dots[2 * c] / op.dots[2 * c + 1] - o.sigma;
        }
    if (info) {
        info->modes = k; info->block = kSpBlock; info->iterations = o.iterations; info->unconverged = o.unconverged;
        info->h_max = o.h_max; info->shift = o.sigma; info->c_max = op.c_max; info->max_residual = o.worst;
        info->setup_ms = o.setup_ms; info->solve_ms = o.solve_ms;
    }
    return rc;
}

}  // namespace score

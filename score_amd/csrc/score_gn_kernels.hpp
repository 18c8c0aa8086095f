// score_gn_kernels.hpp -- device side of the local refinement (score_gn.hpp): per-measurement blocks,
// the gathers that turn them into J'J / J'r on the handle's pattern, trial points.  What a lane does with a
// measurement or a variable is score_gn.hpp's (gn_measurement, gn_retract_variable); the kernels here place the lanes.
// All are small streaming kernels (one measurement / matrix entry / unknown per lane); the work that
// matters -- the damped normal equations -- runs in the solver's own k_factor / k_prec_pre / k_spmv.
#pragma once

#include "score_gn.hpp"
#include "score_kernels.hpp"

namespace score {

// one measurement of the view per lane (gn_measurement): cost (block partial sums) and, with_blocks, its J'J / J'r block
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gn_blocks(GnView v, double* __restrict__ cost_part, int with_blocks) {
    __shared__ double red[8];
    const int64_t m = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const double tot = block_sum(gn_measurement<DIM>(v, m, with_blocks != 0), red);
    if (threadIdx.x == 0) cost_part[blockIdx.x] = tot;
}

// trial point: one pose or landmark per lane, ut = retract(u, step)  (gn_retract_variable; pose 0 has no step)
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gn_trial(const double* __restrict__ u, const double* __restrict__ step,
                                                       double* __restrict__ ut, int64_t Np, int64_t Nl) {
    gn_retract_variable<DIM>(u, step, ut, Np, Nl, (int64_t)blockIdx.x * kThreads + threadIdx.x);
}

// one entry of H per lane: the sum of its block slots in list order (+ lambda on the diagonal)
__global__ __launch_bounds__(kThreads) void k_gn_gather_h(const int32_t* __restrict__ hc_ptr, const int32_t* __restrict__ hc_slot,
                                                          const double* __restrict__ hblk, const int32_t* __restrict__ is_diag,
                                                          double lambda, double* __restrict__ out, int64_t nnz) {
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= nnz) return;
    double acc = 0.0;
    for (int32_t c = hc_ptr[k]; c < hc_ptr[k + 1]; ++c) acc += hblk[hc_slot[c]];
    out[k] = is_diag[k] ? acc + lambda : acc;
}

// one unknown per lane: g = J'r, rhs = -g, block partial of |g|_inf
__global__ __launch_bounds__(kThreads) void k_gn_gather_g(const int32_t* __restrict__ gc_ptr, const int32_t* __restrict__ gc_slot,
                                                          const double* __restrict__ gblk, double* __restrict__ rhs,
                                                          double* __restrict__ gmax_part, int64_t n) {
    __shared__ double red[8];
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double a = 0.0;
    if (i < n) {
        double acc = 0.0;
        for (int32_t c = gc_ptr[i]; c < gc_ptr[i + 1]; ++c) acc += gblk[gc_slot[c]];
        rhs[i] = -acc;
        a = acc == acc ? fabs(acc) : INFINITY;
    }
    const double mx = block_max(a, red);
    if (threadIdx.x == 0) gmax_part[blockIdx.x] = mx;
}

}  // namespace score

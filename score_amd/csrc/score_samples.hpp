// score_samples.hpp -- draws from the Gaussian posterior N(x_hat, H^-1) of the refined estimate (include/score_samples.h):
// perturb-and-solve.  With r the whitened residual of the refinement's cost and J its Jacobian, H = J'J, and for
// z ~ N(0, I) the solution of H delta = J'z has covariance H^-1 J'J H^-1 = H^-1 exactly: no factor of H, no square root.
//
// What exists already and is used as it is: the measurement Jacobians (gn_*_jac of score_gn.hpp, the ones the blocks of
// the refinement are made of), the contribution lists gc_ptr / gc_slot and the layout of gblk, the gather of H, the chain
// factors, and the whole lock-step iteration of score_marginals.hpp (mv_block_pcg: product, step, M^-1, direction, the
// chunked queue, the stopping rule and breakdown words), the counter-based Philox4x32-10 and Box-Muller of
// score_generate.hpp.  New here, per block of up to kMvMaxWidth draws:
//   k_ps_blocks<DIM>  one lane per measurement: J once, then per live draw z (ps_noise) and J'z into the draw's slice of a
//                     block buffer laid out as gblk (gblk_size() doubles per draw)
//   k_ps_gather<NV>   b_c[i] = the sum of unknown i's contributions in list order, all live draws from one pass over the
//                     lists; tiles as the product's (mv_tiles over gc_ptr): short lists four lanes each, a long list (a
//                     landmark ranged from every pose) over the workgroup, both joined in a fixed order -- the tile's body
//                     is ps_gather_tile<NV>, which k_gbs_gather of score_samples_batch.hpp calls too
//   k_ps_probe_begin  once per call: a random vector (ps_probe_value, the group's as well) as the right-hand side of one
//                     probe column, whose iteration says whether H is singular (the draws' own right-hand sides lie in
//                     the range of H and cannot)
//   k_ps_begin        x = 0, r = b_c, the done / iteration words as k_mv_rhs sets them
//   k_ps_residual     partials of |b_c - H x_c|^2
//   k_ps_moments<DIM> per variable M_v += sum_s delta_v delta_v', mean_v += sum_s delta_v over the block's converged draws
//                     in ascending s, into running sums that stay on the device across the blocks
//   k_ps_select       the selected variables' unknowns of every live draw
// No atomics; every sum has a fixed order, so two calls give the same bits and a draw does not depend on its block.
// The call itself (ps_solve) is written once and takes what is done with a solved block as a parameter: the moments and the
// step selection here (PsMoments), the per-measurement sums of score_leverage.hpp.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/score_samples.h"
#include "score_generate.hpp"
#include "score_gn.hpp"

namespace score {

constexpr uint32_t GEN_SAMPLE = 13;  // the Philox purpose of the posterior noise (GenPurpose of score_generate.hpp ends at 12)
constexpr uint32_t GEN_PROBE = 14;   // ... and of the probe vector of ps_solve
constexpr int kPsProbeIters = 4000;  // the probe's own budget: what the refinement gives a linear solve

// component q of measurement m's noise in draw s (the global index): see include/score_samples.h
SCORE_GN_HD double ps_noise(uint64_t seed, int64_t m, int64_t s, int q) {
    double n0, n1;
    gen_normal2(philox4x32_10(seed, GEN_SAMPLE, (uint32_t)m, (uint32_t)s, (uint32_t)(q >> 1)), n0, n1);
    return (q & 1) ? n1 : n0;
}
// the NR components of a measurement, one Philox block per pair
template <int NR>
SCORE_GN_HD void ps_noise_rows(uint64_t seed, int64_t m, int64_t s, double* z) {
#pragma unroll
    for (int h = 0; h < (NR + 1) / 2; ++h) {
        double n0, n1;
        gen_normal2(philox4x32_10(seed, GEN_SAMPLE, (uint32_t)m, (uint32_t)s, (uint32_t)h), n0, n1);
        z[2 * h] = n0;
        if (2 * h + 1 < NR) z[2 * h + 1] = n1;
    }
}

// residual rows of a graph: the length of one draw's noise in the (m, q) order
template <int DIM>
SCORE_GN_HD int64_t ps_rows(int64_t n_rel, int64_t n_rng, int64_t n_pri) { return (DIM + DIM * DIM) * n_rel + n_rng + DIM * n_pri; }

// Measurement m of the view (numbered as gn_measurement numbers them): its Jacobian once, then for the draws
// s0 .. s0 + live - 1 the noise z and J'z into blk + k * gsz (a slice laid out as gblk) and, noise non-null, z into
// noise + k * rows.
template <int DIM>
SCORE_GN_HD void ps_measurement(const GnView& v, int64_t m, uint64_t seed, int64_t s0, int live, double* blk, int64_t gsz, double* noise,
                                int64_t rows) {
    constexpr int PS = DIM == 2 ? 3 : 12, NR = DIM == 2 ? 6 : 12, NG = 2 * DIM;
    if (m < v.n_rel) {
        double r[NR], J[NR][NR];
        const double* pi = v.X + PS * (int64_t)v.meas.rel_i[m];
        const double* pj = v.X + PS * (int64_t)v.meas.rel_j[m];
        if constexpr (DIM == 2)
            gn_rel_jac(pi[0], pi[1], pi[2], pj[0], pj[1], pj[2], v.meas.rel_t + 2 * m, v.meas.rel_R + 4 * m, v.meas.rel_kappa[m],
                       v.meas.rel_tau[m], r, J, true);
        else
            gn_rel_jac3(pi, pj, v.meas.rel_t + 3 * m, v.meas.rel_R + 9 * m, v.meas.rel_kappa[m], v.meas.rel_tau[m], r, J, true);
        for (int k = 0; k < live; ++k) {
            double z[NR], b[NR];
            ps_noise_rows<NR>(seed, m, s0 + k, z);
            gn_jt_vec<NR>(J, z, b);
            gn_store<NR>(blk + (int64_t)k * gsz + NR * m, b);
            if (noise) gn_store<NR>(noise + (int64_t)k * rows + NR * m, z);
        }
    } else if (m < v.n_rel + v.n_rng) {
        const int64_t e = m - v.n_rel;
        double J[NG];
        if constexpr (DIM == 2) {
            const double* pa = gn_point2(v.X, v.Np, v.meas.rng_a[e]);
            const double* pb = gn_point2(v.X, v.Np, v.meas.rng_b[e]);
            (void)gn_range_jac(pa[0], pa[1], pb[0], pb[1], v.meas.rng_dist[e], v.meas.rng_prec[e], J, true);
        } else {
            const double* pa = gn_point3(v.X, v.Np, v.meas.rng_a[e]);
            const double* pb = gn_point3(v.X, v.Np, v.meas.rng_b[e]);
            const double a3[3] = {pa[0], pa[1], pa[2]}, b3[3] = {pb[0], pb[1], pb[2]};
            (void)gn_range_jac3(a3, b3, v.meas.rng_dist[e], v.meas.rng_prec[e], J, true);
        }
        for (int k = 0; k < live; ++k) {
            const double z = ps_noise(seed, m, s0 + k, 0);
            double b[NG];
#pragma unroll
            for (int a = 0; a < NG; ++a) b[a] = J[a] * z;
            gn_store<NG>(blk + (int64_t)k * gsz + NR * v.n_rel + NG * e, b);
            if (noise) noise[(int64_t)k * rows + NR * v.n_rel + e] = z;
        }
    } else if (m < v.n_rel + v.n_rng + v.n_pri) {
        const int64_t e = m - v.n_rel - v.n_rng;
        const double* l = v.X + PS * v.Np + DIM * (int64_t)v.meas.pri_l[e];
        double r[DIM], sw;
        if constexpr (DIM == 2) {
            sw = gn_prior_jac(l[0], l[1], v.meas.pri_t + 2 * e, v.meas.pri_prec[e], r);
        } else {
            const double l3[3] = {l[0], l[1], l[2]};
            sw = gn_prior_jac3(l3, v.meas.pri_t + 3 * e, v.meas.pri_prec[e], r);
        }
        for (int k = 0; k < live; ++k) {
            double z[DIM], b[DIM];
            ps_noise_rows<DIM>(seed, m, s0 + k, z);
#pragma unroll
            for (int a = 0; a < DIM; ++a) b[a] = sw * z[a];
            gn_store<DIM>(blk + (int64_t)k * gsz + NR * v.n_rel + NG * v.n_rng + DIM * e, b);
            if (noise) gn_store<DIM>(noise + (int64_t)k * rows + NR * v.n_rel + v.n_rng + DIM * e, z);
        }
    }
}

}  // namespace score

#if defined(__HIPCC__)

#include "score_marginals.hpp"

namespace score {

struct PsArgs {
    GnView v;                  // the graph at the point (its hblk / gblk are not touched)
    uint64_t seed;
    long long s0;              // global index of the block's first draw
    int live;                  // the block's draws
    double* blk;               // [k * gsz + slot]: J'z of draw k, laid out as gblk
    long long gsz, rows, n;
    double* noise;             // [k * rows + row] or null
    const int32_t* gc_ptr; const int32_t* gc_slot;
    const int4* tiles;         // of the gather: {first unknown, end unknown, long list?, 0}
    double* b;                 // [k * n + i]
    unsigned take;             // moments: bit k set -- draw k enters the sums
    const double* x;           // [k * n + i]: the block's solutions
    double* mom; double* mean; // the running sums
};

// one measurement per lane (ps_measurement)
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_ps_blocks(PsArgs a) {
    ps_measurement<DIM>(a.v, (int64_t)blockIdx.x * kThreads + threadIdx.x, a.seed, (int64_t)a.s0, a.live, a.blk, (int64_t)a.gsz, a.noise,
                        (int64_t)a.rows);
}

// The gather of one tile of unknowns: b_c[i] = sum of blk_c[gc_slot[.]] over the list of i, the draws c < live.  Stated once:
// k_ps_gather (the draws of one graph) and k_gbs_gather (score_samples_batch.hpp: the live slots of the tile's member) call
// it with their count.  A short list is summed by kMvLanes lanes (entries sub, sub + 4, ... each in list order), joined as
// (l0 + l1) + (l2 + l3); a long list by the workgroup (entries t, t + 256, ...), joined by the wave's tree and then
// (w0 + w1) + (w2 + w3).  red: (kMvThreads / 64) * NV doubles of LDS.  Every lane enters with the same tile and live > 0.
template <int NV>
__device__ __forceinline__ void ps_gather_tile(const int32_t* gc_ptr, const int32_t* gc_slot, const int4 tile, const double* blk,
                                               const long long gsz, double* b, const long long n, const int live, double* red) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double acc[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) acc[c] = 0.0;
    if (tile.z) {
        const int row = tile.x;
        const int k1 = gc_ptr[row + 1];
        for (int k = gc_ptr[row] + t; k < k1; k += kMvThreads) {
            const long long slot = gc_slot[k];
#pragma unroll
            for (int c = 0; c < NV; ++c)
                if (c < live) acc[c] += blk[c * gsz + slot];
        }
#pragma unroll
        for (int c = 0; c < NV; ++c)
            if (c < live) {
                const double s = wave_sum(acc[c]);
                if (lane == 0) red[wave * NV + c] = s;
            }
        __syncthreads();
        if (t < NV && t < live) b[t * n + row] = (red[t] + red[NV + t]) + (red[2 * NV + t] + red[3 * NV + t]);
        return;
    }
    const int row = tile.x + t / kMvLanes, sub = t % kMvLanes;
    const bool mine = row < tile.y;
    if (mine) {
        const int k1 = gc_ptr[row + 1];
        for (int k = gc_ptr[row] + sub; k < k1; k += kMvLanes) {
            const long long slot = gc_slot[k];
#pragma unroll
            for (int c = 0; c < NV; ++c)
                if (c < live) acc[c] += blk[c * gsz + slot];
        }
    }
#pragma unroll
    for (int c = 0; c < NV; ++c)
        if (c < live) {
            double s = acc[c];
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            if (mine && sub == 0) b[c * n + row] = s;
        }
}

// one tile of unknowns per workgroup, the block's draws
template <int NV>
__global__ __launch_bounds__(kMvThreads) void k_ps_gather(PsArgs a) {
    __shared__ double red[(kMvThreads / 64) * NV];
    ps_gather_tile<NV>(a.gc_ptr, a.gc_slot, a.tiles[blockIdx.x], a.blk, a.gsz, a.b, a.n, a.live, red);
}

// the probe's value of unknown i (member-local in a group): one standard normal of the Philox stream GEN_PROBE of (seed, i)
__device__ __forceinline__ double ps_probe_value(uint64_t seed, long long i) {
    double n0, n1;
    gen_normal2(philox4x32_10(seed, GEN_PROBE, (uint32_t)i, 0u, 0u), n0, n1);
    return n0;
}

// grid (row blocks, columns): x = 0, r = b_c (columns beyond `live`: zero, done from the start)
__global__ __launch_bounds__(kMvThreads) void k_ps_begin(MvArgs a, const double* __restrict__ b) {
    const int c = blockIdx.y, t = threadIdx.x;
    const long long i = (long long)blockIdx.x * kMvThreads + t;
    const bool on = c < a.live;
    if (i < a.n) {
        a.x[c * a.n + i] = 0.0;
        a.r[c * a.n + i] = on ? b[c * a.n + i] : 0.0;
    }
    if (blockIdx.x == 0 && t == 0) {
        a.flags[kMvDone + c] = on ? 0 : 1;
        a.flags[kMvIters + c] = 0;
        if (c == 0) a.flags[kMvZero] = 0;
    }
}

// grid (row blocks, columns): the probe -- x = 0, r = b = one standard normal per unknown in column 0, the other columns done
__global__ __launch_bounds__(kMvThreads) void k_ps_probe_begin(MvArgs a, uint64_t seed, double* __restrict__ b) {
    const int c = blockIdx.y, t = threadIdx.x;
    const long long i = (long long)blockIdx.x * kMvThreads + t;
    const bool on = c == 0;
    if (i < a.n) {
        const double n0 = on ? ps_probe_value(seed, i) : 0.0;
        a.x[c * a.n + i] = 0.0;
        a.r[c * a.n + i] = n0;
        b[c * a.n + i] = n0;
    }
    if (blockIdx.x == 0 && t == 0) {
        a.flags[kMvDone + c] = on ? 0 : 1;
        a.flags[kMvIters + c] = 0;
        if (c == 0) a.flags[kMvZero] = 0;
    }
}

// grid (row blocks, live columns): partials of |b_c - w_c|^2 with w = H x
__global__ __launch_bounds__(kMvThreads) void k_ps_residual(MvArgs a, const double* __restrict__ b) {
    __shared__ double red[4];
    const int c = blockIdx.y, t = threadIdx.x;
    const long long i = (long long)blockIdx.x * kMvThreads + t;
    double d = 0.0;
    if (i < a.n) d = b[c * a.n + i] - a.w[c * a.n + i];
    const double s = block_sum(d * d, red);
    if (t == 0) a.res_part[(size_t)c * gridDim.x + blockIdx.x] = s;
}

// the K unknowns from `first` of one variable: its running sums take the draws of `take` in ascending order
template <int K>
__device__ __forceinline__ void ps_accumulate(const PsArgs& a, long long first, double* mom, double* mean) {
    double M[K * K], mu[K];
#pragma unroll
    for (int e = 0; e < K * K; ++e) M[e] = mom[e];
#pragma unroll
    for (int e = 0; e < K; ++e) mu[e] = mean[e];
    for (int c = 0; c < a.live; ++c) {
        if (!(a.take >> c & 1)) continue;
        double d[K];
#pragma unroll
        for (int e = 0; e < K; ++e) d[e] = a.x[c * a.n + first + e];
#pragma unroll
        for (int p = 0; p < K; ++p) {
            mu[p] += d[p];
#pragma unroll
            for (int q = 0; q < K; ++q) M[p * K + q] += d[p] * d[q];
        }
    }
#pragma unroll
    for (int e = 0; e < K * K; ++e) mom[e] = M[e];
#pragma unroll
    for (int e = 0; e < K; ++e) mean[e] = mu[e];
}

// one variable with unknowns per lane: poses 1..Np-1 (DP x DP), then the landmarks (DIM x DIM)
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_ps_moments(PsArgs a) {
    constexpr int DP = DIM == 2 ? 3 : 6;
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x, np = a.v.Np - 1;
    if (i < np) {
        ps_accumulate<DP>(a, DP * i, a.mom + DP * DP * i, a.mean + DP * i);
    } else if (i < np + a.v.Nl) {
        const long long l = i - np;
        ps_accumulate<DIM>(a, DP * np + DIM * l, a.mom + DP * DP * np + DIM * DIM * l, a.mean + DP * np + DIM * l);
    }
}

// grid (blocks over the C selected unknowns, live columns): steps[c, s] = x_c[sel[s]]
__global__ __launch_bounds__(kMvThreads) void k_ps_select(MvArgs a, double* __restrict__ steps) {
    const int c = blockIdx.y;
    const long long s = (long long)blockIdx.x * kMvThreads + threadIdx.x;
    if (s < a.C) steps[(long long)c * a.C + s] = a.x[c * a.n + a.sel[s]];
}

// The draws' buffers: they stay with the refinement handle between calls, as MvWork's do.
struct PsWork {
    DevBuf<double> blk, b, mom, mean, noise;
    MvTiles tiles;  // of the gather, cut from the contribution lists
    void reserve(const GnProblem& P, bool with_noise, int64_t rows, hipStream_t st) {
        NoArena no_arena;
        if (!blk.d) {
            tiles.add(P.gc_ptr, P.n);
            tiles.send(st);
            const size_t nv = (size_t)kMvMaxWidth;
            blk.alloc(nv * (size_t)std::max<int64_t>(1, P.gblk_size())); blk.zero(st);
            b.alloc(nv * (size_t)P.n); b.zero(st);
            const int64_t dp = P.dp(), d = P.dim;
            mom.alloc((size_t)(dp * dp * (P.Np - 1) + d * d * P.Nl));
            mean.alloc((size_t)P.n);
        }
        if (with_noise && !noise.d) { noise.alloc((size_t)kMvMaxWidth * (size_t)std::max<int64_t>(1, rows)); noise.zero(st); }
    }
};

// What score_refine_samples does with a solved block -- the consumer ps_solve is given: the per-variable moments of the
// converged draws and the selected variables' steps.
struct PsMoments {
    const int32_t* vars; int32_t n_vars;
    double* moments; double* means; double* steps;
    std::vector<int32_t> sel;
    int C = 0;
    DevBuf<int32_t> d_sel;
    DevBuf<double> d_steps;
    PsWork* Q = nullptr;
    unsigned n_vblocks = 1;
    void check(const GnProblem& P, const std::string& who) {
        if (n_vars < 0 || (n_vars > 0 && !vars)) throw std::runtime_error(who + "n_vars variables without their list");
        if (n_vars > 0) mv_variable_unknowns(P.Np, P.Nl, P.dp(), P.dim, vars, n_vars, who, sel);
        C = (int)sel.size();
        n_vblocks = (unsigned)std::max<int64_t>(1, (P.Np - 1 + P.Nl + kThreads - 1) / kThreads);
    }
    template <class Refine>
    void begin(Refine& R, PsArgs& q, MvArgs& a, hipStream_t st) {
        Q = &R.ps;
        Q->mom.zero(st); Q->mean.zero(st);
        if (C) {
            NoArena no_arena;
            d_sel.alloc((size_t)C); d_steps.alloc((size_t)kMvMaxWidth * (size_t)C);
            staged_h2d(d_sel.d, sel.data(), (size_t)C * sizeof(int32_t), st);
        }
        a.sel = d_sel.d; a.C = C;
        q.mom = Q->mom.d; q.mean = Q->mean.d;
    }
    template <class Refine>
    void block(Refine& R, const PsArgs& q, const MvArgs& a, int k0, int live, hipStream_t st) {
        if (q.take) {
            gn_dim(R.P.dim, [&](auto dim) { hipLaunchKernelGGL(k_ps_moments<decltype(dim)::value>, dim3(n_vblocks), dim3(kThreads), 0, st, q); });
        }
        if (C) {
            hipLaunchKernelGGL(k_ps_select, dim3((unsigned)((C + kMvThreads - 1) / kMvThreads), (unsigned)live), dim3(kMvThreads), 0, st, a, d_steps.d);
            if (steps) staged_d2h(steps + (size_t)k0 * (size_t)C, d_steps.d, (size_t)live * (size_t)C * sizeof(double), st);
        }
    }
    void end(hipStream_t st) {
        if (moments) staged_d2h(moments, Q->mom.d, Q->mom.n * sizeof(double), st);
        if (means) staged_d2h(means, Q->mean.d, Q->mean.n * sizeof(double), st);
    }
};

// The draws of a call: the probe, then block after block the noise, J'z, the lock-step solve, the true residuals and the
// verdict of every draw.  Refine: score_refine (its point, blocks and gather, its linear-mode handle, its MvWork and PsWork).
// What is done with a solved block is the caller's (use): check(P, who) before any device work, begin(R, q, a, st) once the
// buffers stand, block(R, q, a, k0, live, st) after the block's verdict -- q.take holds the draws that converged, q.live the
// block's draws, q.x its solutions -- and end(st) before the clock stops.  score_refine_samples passes PsMoments,
// score_refine_leverage (score_leverage.hpp) its per-measurement sums.
template <class Refine, class Use>
int ps_solve(Refine& R, const std::string& who, const double* poses, const double* landmarks, uint64_t seed, int64_t first_sample,
             int32_t n_samples, double rel_tol, int32_t max_iters, int32_t block_width, double* rhs, double* noise, double* residuals,
             int32_t* iters, score_samples_info* info, Use& use) {
    const GnProblem& P = R.P;
    if (n_samples < 1) throw std::runtime_error(who + "n_samples must be >= 1");
    if (block_width < 1 || block_width > kMvMaxWidth) throw std::runtime_error(who + "block_width must be 1..16");
    if (!(rel_tol > 0.0) || max_iters < 1) throw std::runtime_error(who + "rel_tol must be positive and max_iters >= 1");
    if (first_sample < 0 || first_sample + (int64_t)n_samples > ((int64_t)1 << 32)) throw std::runtime_error(who + "draw indices must lie in 0 .. 2^32 - 1");
    use.check(P, who);
    HipBackend& be = R.be();
    hipStream_t st = R.stream();
    const long long n = P.n;
    const double t0 = now_ms();
    // H at the point on the handle's pattern, the chains factored once: as mv_solve
    R.h_at_point(poses, landmarks, who, "blocks of draws need");
    be.derive_rho_data(false);
    const int NV = mv_slots(block_width);
    const int64_t rows = gn_dim(P.dim, [&](auto dim) { return ps_rows<decltype(dim)::value>(P.n_rel(), P.n_rng(), P.n_pri()); });
    auto& W = R.mv;
    auto& Q = R.ps;
    W.reserve(P, R.product_tiles(), be.n_prec, be.H->bs * be.n_join_seps, st);
    Q.reserve(P, noise != nullptr, rows, st);
    const int n_rblocks = (int)((n + kMvThreads - 1) / kMvThreads);
    MvArgs a = mv_block_args(be, W, n, rel_tol);
    PsArgs q{};
    q.v = R.view(R.u.d); q.seed = seed; q.blk = Q.blk.d; q.gsz = P.gblk_size(); q.rows = rows; q.n = n;
    q.noise = noise ? Q.noise.d : nullptr;
    q.gc_ptr = R.gc_ptr.d; q.gc_slot = R.gc_slot.d; q.tiles = Q.tiles.dev.d; q.b = Q.b.d; q.x = W.x.d;
    use.begin(R, q, a, st);
    std::vector<int32_t> flags((size_t)kMvFlagWords);
    // Is H singular?  The draws cannot tell: b = J'z lies in the range of J'J, so the iteration converges on a singular H as
    // well and returns draws without a component along the directions the measurements leave open.  One more column can: a
    // random vector has a component there, H x = xi is then inconsistent and its iteration stalls or breaks down.  Such a
    // call reports every draw as not converged.
    // The done word alone is no verdict there (a breakdown step can leave a tiny recurrence residual beside a true one of
    // the right-hand side's size), so the probe's TRUE residual decides: |xi - H x|_2 <= sqrt(rel_tol) |xi|_2.  The rule
    // bounds r'M^-1 r, which lets the Euclidean residual of a converged column exceed rel_tol |xi| by sqrt(cond M) at most;
    // a singular H leaves xi's component along the open directions, |xi| / sqrt(n) per direction on average; sqrt(rel_tol)
    // lies between the two as long as n < 1 / rel_tol.
    a.c0 = 0; a.live = 1;
    hipLaunchKernelGGL(k_ps_probe_begin, dim3((unsigned)n_rblocks, (unsigned)NV), dim3(kMvThreads), 0, st, a, seed, Q.b.d);
    std::vector<double> probe_part((size_t)n_rblocks);
    auto probe_norm2 = [&](const MvArgs& m) {  // |xi - m.w|^2 of column 0
        hipLaunchKernelGGL(k_ps_residual, dim3((unsigned)n_rblocks, 1u), dim3(kMvThreads), 0, st, m, (const double*)Q.b.d);
        HIP_CHECK(hipGetLastError());
        staged_d2h(probe_part.data(), W.res_part.d, (size_t)n_rblocks * sizeof(double), st);
        double t = 0.0;
        for (double v : probe_part) t += v;
        return t;
    };
    MvArgs at_zero = a;
    at_zero.w = W.x.d;  // (x = 0: |xi|^2)
    const double xi2 = probe_norm2(at_zero);
    mv_block_pcg(be, W, a, NV, n_rblocks, kPsProbeIters, flags, st);
    a.all_columns = 1; a.p_in = W.x.d;
    mv_launch_product(a, NV, st);
    const double probe2 = probe_norm2(a);
    const bool determined = flags[(size_t)kMvDone] == 1 && std::isfinite(probe2) && probe2 <= rel_tol * xi2;
    HIP_CHECK(sync_stream(st));
    const double t1 = now_ms();
    std::vector<int32_t> s_done((size_t)n_samples, 0), s_iters((size_t)n_samples, 0);
    std::vector<double> res_part((size_t)NV * (size_t)n_rblocks), s_res((size_t)n_samples, 0.0);
    int batches = 0, pcg_iters = 0;
    double rhs_ms = 0.0;
    for (int k0 = 0; k0 < n_samples; k0 += block_width) {
        const int live = std::min<int>(block_width, n_samples - k0);
        a.c0 = 0; a.live = live;
        q.s0 = first_sample + k0; q.live = live;
        // the block's noise and right-hand sides
        const double tb = now_ms();
        gn_dim(P.dim, [&](auto dim) { hipLaunchKernelGGL(k_ps_blocks<decltype(dim)::value>, dim3((unsigned)R.n_mblocks), dim3(kThreads), 0, st, q); });
        mv_with_slots(NV, [&](auto nv) {
            hipLaunchKernelGGL(k_ps_gather<decltype(nv)::value>, dim3((unsigned)Q.tiles.n), dim3(kMvThreads), 0, st, q);
        });
        hipLaunchKernelGGL(k_ps_begin, dim3((unsigned)n_rblocks, (unsigned)NV), dim3(kMvThreads), 0, st, a, (const double*)Q.b.d);
        HIP_CHECK(hipGetLastError());
        if (noise) staged_d2h(noise + (size_t)k0 * (size_t)rows, Q.noise.d, (size_t)live * (size_t)rows * sizeof(double), st);
        if (rhs) staged_d2h(rhs + (size_t)k0 * (size_t)n, Q.b.d, (size_t)live * (size_t)n * sizeof(double), st);
        HIP_CHECK(sync_stream(st));
        rhs_ms += now_ms() - tb;
        mv_block_pcg(be, W, a, NV, n_rblocks, max_iters, flags, st);
        // the true residual of every draw of the block (one more product, w = H x)
        a.all_columns = 1; a.p_in = W.x.d;
        mv_launch_product(a, NV, st);
        hipLaunchKernelGGL(k_ps_residual, dim3((unsigned)n_rblocks, (unsigned)live), dim3(kMvThreads), 0, st, a, (const double*)Q.b.d);
        HIP_CHECK(hipGetLastError());
        staged_d2h(res_part.data(), W.res_part.d, (size_t)live * (size_t)n_rblocks * sizeof(double), st);
        int most = 0;
        unsigned take = 0;
        for (int c = 0; c < live; ++c) {
            double s = 0.0;
            for (int b = 0; b < n_rblocks; ++b) s += res_part[(size_t)c * (size_t)n_rblocks + (size_t)b];
            const double rho = std::sqrt(s);
            const bool ok = determined && flags[(size_t)(kMvDone + c)] == 1 && std::isfinite(rho);
            s_res[(size_t)(k0 + c)] = rho;
            s_done[(size_t)(k0 + c)] = ok ? 1 : 0;
            s_iters[(size_t)(k0 + c)] = flags[(size_t)(kMvIters + c)];
            most = std::max(most, flags[(size_t)(kMvIters + c)]);
            if (ok) take |= 1u << c;
        }
        q.take = take;
        use.block(R, q, a, k0, live, st);
        HIP_CHECK(hipGetLastError());
        pcg_iters += most;
        ++batches;
    }
    use.end(st);
    HIP_CHECK(sync_stream(st));
    const double t2 = now_ms();
    double worst = 0.0;
    const int unconverged = mv_report(s_done, s_iters, s_res, residuals, iters, worst);
    if (info) {
        info->samples = n_samples; info->batches = batches; info->pcg_iters = pcg_iters; info->unconverged = unconverged;
        info->max_residual = worst; info->setup_ms = t1 - t0; info->rhs_ms = rhs_ms; info->solve_ms = t2 - t1 - rhs_ms;
    }
    return unconverged ? 1 : 0;
}

}  // namespace score

#endif  // __HIPCC__

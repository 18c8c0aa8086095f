// score_leverage.hpp -- leverage of the measurements and predicted range variances at the refined estimate
// (include/score_leverage.h).  With delta = H^-1 J'z a posterior draw (score_samples.hpp), J delta = P z for the hat matrix
// P = J H^-1 J': over the rows of measurement m, E |J_m delta|^2 = h_m (its leverage) and E |z_m - J_m delta|^2 = rows_m - h_m
// (its redundancy).  Both are sums over the draws ps_solve produces anyway, so score_refine_leverage is ps_solve with another
// consumer of a solved block; the exact variance of a LISTED hypothetical range, g'H^-1 g, is one column H x = g of the
// marginals' lock-step iteration (mv_block_pcg).
//
// What exists already and is used as it is: the draws (ps_solve: noise, J'z, probe, iteration, verdicts), the measurement
// Jacobians (gn_*_jac, the ones ps_measurement calls), the counter-based noise (ps_noise_rows / ps_noise: z is regenerated, not
// stored), the iteration, the product and the residual partials (mv_block_pcg, mv_launch_product, k_ps_residual).  New here:
//   k_lv_measure<DIM>   one lane per measurement, then one per listed pair: J (or g) once, then per converged draw of the
//                       block, ascending, y = J_m delta at the measurement's own unknowns, z again, and t = |y|^2, t^2,
//                       v = |z - y|^2, v^2 into running sums held in registers (read before the loop, stored after it: the
//                       sums stay on the device across the blocks)
//   k_lv_pair_rhs<DIM>  x = 0, r = b = g_c for the block's live pairs, the done / iteration words as k_mv_rhs sets them
//   k_lv_pair_dot<DIM>  variances[c] = g_c'x_c from its at most 2 DIM entries, distances[c]
// No atomics and a fixed order: two calls give the same bits, and a measurement's sums do not depend on block_width.
// What a lane of these kernels does is stated once, as __device__ functions on a GnView (lv_measure_lane, lv_pair_lane,
// lv_pair_entry, lv_pair_dot_lane): the kernels here call them for a graph, score_leverage_batch.hpp's for a member of a group.
//
// Access pattern of k_lv_measure.  A lane reads delta only at its measurement's unknowns -- pose p >= 1 at DP (p - 1),
// landmark l at DP (Np - 1) + DIM l, pose 0 nowhere -- ONCE per draw, before the rows are formed.  Consecutive relative
// poses are consecutive odometry steps, so a wave's pose reads are contiguous; the ranges of a graph with few beacons end at
// the same landmark for whole waves, whose lanes then read one address (a broadcast, one transaction per wave and draw).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/score_leverage.h"
#include "score_samples.hpp"

namespace score {

// first unknown of pose p (its DP unknowns follow), -1 for the fixed pose 0
template <int DIM>
SCORE_GN_HD long long lv_pose_first(int64_t p) {
    constexpr int DP = DIM == 2 ? 3 : 6;
    return p >= 1 ? (long long)DP * (p - 1) : -1;
}
// first translation unknown of a range endpoint v (variable id: pose or landmark; DIM unknowns follow), -1 for pose 0
template <int DIM>
SCORE_GN_HD long long lv_point_first(int64_t Np, int64_t v) {
    constexpr int DP = DIM == 2 ? 3 : 6;
    if (v >= Np) return (long long)DP * (Np - 1) + (long long)DIM * (v - Np);
    return v >= 1 ? (long long)DP * (v - 1) + (DP - DIM) : -1;
}
// the hypothetical range a - b at the view's point: u (DIM) = the unit vector of p_a - p_b by the rule of gn_range_jac (a range
// of precision 1 and measured distance 0: its Jacobian is (u, -u), its residual the distance); returns |p_a - p_b|
template <int DIM>
SCORE_GN_HD double lv_pair_direction(const GnView& v, int64_t a, int64_t b, double* u) {
    double J[2 * DIM], rho;
    if constexpr (DIM == 2) {
        const double* pa = gn_point2(v.X, v.Np, a);
        const double* pb = gn_point2(v.X, v.Np, b);
        rho = gn_range_jac(pa[0], pa[1], pb[0], pb[1], 0.0, 1.0, J, true);
    } else {
        const double* pa = gn_point3(v.X, v.Np, a);
        const double* pb = gn_point3(v.X, v.Np, b);
        const double a3[3] = {pa[0], pa[1], pa[2]}, b3[3] = {pb[0], pb[1], pb[2]};
        rho = gn_range_jac3(a3, b3, 0.0, 1.0, J, true);
    }
#pragma unroll
    for (int k = 0; k < DIM; ++k) u[k] = J[k];
    return rho;
}

}  // namespace score

#if defined(__HIPCC__)

namespace score {

struct LvArgs {
    GnView v;                  // the graph at the point
    uint64_t seed;
    long long s0;              // global index of the block's first draw
    int live;                  // the block's draws
    unsigned take;             // bit c set: draw c enters the sums
    const double* x;           // [c * n + i]: the block's solutions
    long long n, M;            // unknowns, measurements
    double* sums;              // [k * M + m], k = 0..3: the running sums of t, t^2, v, v^2
    const int32_t* pa; const int32_t* pb;
    int n_pairs;
    double* pair_sums;         // [k * n_pairs + c], k = 0..1: of (g_c'delta)^2 and its square
};

// a block of pairs of lv_pair_solve
struct LvPairArgs {
    GnView v;                  // the graph at the point
    const double* x;           // [c * n + i]: the block's solutions
    long long n;
    const int32_t* pa; const int32_t* pb;
    int c0, live;              // the block's first pair, its pairs
    double* b;                 // [c * n + i]: g of the block's pair c
    double* var; double* dist; // per pair
};

// the K unknowns from `first` of column c of x (none: zeros) -- read once per draw
template <int K>
__device__ __forceinline__ void lv_read(const double* x, long long n, int c, long long first, double* d) {
#pragma unroll
    for (int e = 0; e < K; ++e) d[e] = first >= 0 ? x[c * n + first + e] : 0.0;
}

// four running sums of one measurement: in before the loop over the draws, out after it.  sums: the lane's own entry of the
// first sum, the other three `stride` apart (consecutive lanes, consecutive entries: a wave's loads and stores coalesce)
struct LvSums {
    double t1, t2, v1, v2;
    __device__ __forceinline__ void load(const double* sums, long long stride) {
        t1 = sums[0]; t2 = sums[stride]; v1 = sums[2 * stride]; v2 = sums[3 * stride];
    }
    __device__ __forceinline__ void add(double t, double v) { t1 += t; t2 += t * t; v1 += v; v2 += v * v; }
    __device__ __forceinline__ void store(double* sums, long long stride) const {
        sums[0] = t1; sums[stride] = t2; sums[2 * stride] = v1; sums[3 * stride] = v2;
    }
};

// What one lane does for measurement m of the view (numbered as ps_measurement numbers them; m beyond them: nothing) --
// stated once for a graph (k_lv_measure) and for a member of a group (k_gbl_measure of score_leverage_batch.hpp).  x: column
// c of the block's solutions from x[c * n] (a member's: from its first unknown); seed: the noise stream; s0: the draw of
// column 0; live / take: the block's columns and those that enter the sums; sums / stride: as LvSums.
template <int DIM>
__device__ __forceinline__ void lv_measure_lane(const GnView& v, const long long m, const double* x, const long long n, const uint64_t seed,
                                                const long long s0, const int live, const unsigned take, double* sums, const long long stride) {
    constexpr int PS = DIM == 2 ? 3 : 12, DP = DIM == 2 ? 3 : 6, NR = 2 * DP, NG = 2 * DIM;
    sums += m;
    if (m < v.n_rel) {
        double r[NR], J[NR][NR];
        const double* pi = v.X + PS * (int64_t)v.meas.rel_i[m];
        const double* pj = v.X + PS * (int64_t)v.meas.rel_j[m];
        if constexpr (DIM == 2)
            gn_rel_jac(pi[0], pi[1], pi[2], pj[0], pj[1], pj[2], v.meas.rel_t + 2 * m, v.meas.rel_R + 4 * m, v.meas.rel_kappa[m],
                       v.meas.rel_tau[m], r, J, true);
        else
            gn_rel_jac3(pi, pj, v.meas.rel_t + 3 * m, v.meas.rel_R + 9 * m, v.meas.rel_kappa[m], v.meas.rel_tau[m], r, J, true);
        const long long fi = lv_pose_first<DIM>(v.meas.rel_i[m]), fj = lv_pose_first<DIM>(v.meas.rel_j[m]);
        LvSums S;
        S.load(sums, stride);
        for (int c = 0; c < live; ++c) {
            if (!(take >> c & 1)) continue;
            double d[NR], z[NR];
            lv_read<DP>(x, n, c, fi, d);
            lv_read<DP>(x, n, c, fj, d + DP);
            ps_noise_rows<NR>(seed, m, s0 + c, z);
            double t = 0.0, w = 0.0;
#pragma unroll
            for (int q = 0; q < NR; ++q) {
                double y = 0.0;
#pragma unroll
                for (int e = 0; e < NR; ++e) y += J[q][e] * d[e];
                const double o = z[q] - y;
                t += y * y;
                w += o * o;
            }
            S.add(t, w);
        }
        S.store(sums, stride);
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
        const long long fa = lv_point_first<DIM>(v.Np, v.meas.rng_a[e]), fb = lv_point_first<DIM>(v.Np, v.meas.rng_b[e]);
        LvSums S;
        S.load(sums, stride);
        for (int c = 0; c < live; ++c) {
            if (!(take >> c & 1)) continue;
            double d[NG];
            lv_read<DIM>(x, n, c, fa, d);
            lv_read<DIM>(x, n, c, fb, d + DIM);
            double y = 0.0;
#pragma unroll
            for (int k = 0; k < NG; ++k) y += J[k] * d[k];
            const double o = ps_noise(seed, m, s0 + c, 0) - y;
            S.add(y * y, o * o);
        }
        S.store(sums, stride);
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
        const long long fl = lv_point_first<DIM>(v.Np, v.Np + (int64_t)v.meas.pri_l[e]);
        LvSums S;
        S.load(sums, stride);
        for (int c = 0; c < live; ++c) {
            if (!(take >> c & 1)) continue;
            double d[DIM], z[DIM];
            lv_read<DIM>(x, n, c, fl, d);
            ps_noise_rows<DIM>(seed, m, s0 + c, z);
            double t = 0.0, w = 0.0;
#pragma unroll
            for (int k = 0; k < DIM; ++k) {
                const double y = sw * d[k], o = z[k] - y;
                t += y * y;
                w += o * o;
            }
            S.add(t, w);
        }
        S.store(sums, stride);
    }
}

// What one lane does for the listed pair ia - ib of the view: (g'delta)^2 and its square over the taken columns into *s1 / *s2
// (x, n, live, take: as lv_measure_lane) -- stated once for a graph and for a group (k_gbl_pairs).
template <int DIM>
__device__ __forceinline__ void lv_pair_lane(const GnView& v, const int64_t ia, const int64_t ib, const double* x, const long long n,
                                             const int live, const unsigned take, double* s1_at, double* s2_at) {
    constexpr int NG = 2 * DIM;
    double u[DIM];
    (void)lv_pair_direction<DIM>(v, ia, ib, u);
    const long long fa = lv_point_first<DIM>(v.Np, ia), fb = lv_point_first<DIM>(v.Np, ib);
    double s1 = *s1_at, s2 = *s2_at;
    for (int c = 0; c < live; ++c) {
        if (!(take >> c & 1)) continue;
        double d[NG];
        lv_read<DIM>(x, n, c, fa, d);
        lv_read<DIM>(x, n, c, fb, d + DIM);
        double y = 0.0;
#pragma unroll
        for (int k = 0; k < DIM; ++k) y += u[k] * d[k];
#pragma unroll
        for (int k = 0; k < DIM; ++k) y += -u[k] * d[DIM + k];
        const double t = y * y;
        s1 += t;
        s2 += t * t;
    }
    *s1_at = s1; *s2_at = s2;
}

// One lane per measurement, then one lane per listed pair.
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_lv_measure(LvArgs a) {
    const long long m = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (m < a.M) {
        lv_measure_lane<DIM>(a.v, m, a.x, a.n, a.seed, a.s0, a.live, a.take, a.sums, a.M);
    } else if (m < a.M + a.n_pairs) {
        const long long p = m - a.M;
        lv_pair_lane<DIM>(a.v, a.pa[p], a.pb[p], a.x, a.n, a.live, a.take, a.pair_sums + p, a.pair_sums + a.n_pairs + p);
    }
}

// entry i of g of the pair ia - ib: +u on the translation unknowns of a, -u on those of b, zero elsewhere
template <int DIM>
__device__ __forceinline__ double lv_pair_entry(const GnView& v, const int64_t ia, const int64_t ib, const long long i) {
    const long long fa = lv_point_first<DIM>(v.Np, ia), fb = lv_point_first<DIM>(v.Np, ib);
    const bool at_a = fa >= 0 && i >= fa && i < fa + DIM, at_b = fb >= 0 && i >= fb && i < fb + DIM;
    if (!at_a && !at_b) return 0.0;
    double u[DIM];
    (void)lv_pair_direction<DIM>(v, ia, ib, u);
    double g = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        if (at_a && i == fa + k) g = u[k];
        if (at_b && i == fb + k) g = -u[k];
    }
    return g;
}

// grid (row blocks, columns): x = 0, r = b = g of pair c0 + c (columns beyond `live`: zero, done from the start)
template <int DIM>
__global__ __launch_bounds__(kMvThreads) void k_lv_pair_rhs(MvArgs m, LvPairArgs a) {
    const int c = blockIdx.y, t = threadIdx.x;
    const long long i = (long long)blockIdx.x * kMvThreads + t;
    const bool on = c < a.live;
    if (i < a.n) {
        const double g = on ? lv_pair_entry<DIM>(a.v, a.pa[a.c0 + c], a.pb[a.c0 + c], i) : 0.0;
        m.x[c * a.n + i] = 0.0;
        m.r[c * a.n + i] = g;
        a.b[c * a.n + i] = g;
    }
    if (blockIdx.x == 0 && t == 0) {
        m.flags[kMvDone + c] = on ? 0 : 1;
        m.flags[kMvIters + c] = 0;
        if (c == 0) m.flags[kMvZero] = 0;
    }
}

// What one lane does for a solved pair ia - ib of the view, its solution in column c of x: *var = g'x over the entries of g in
// the order (a's, then b's), *dist = |p_a - p_b| -- stated once for a graph and for a group (k_gbl_pair_dot).
template <int DIM>
__device__ __forceinline__ void lv_pair_dot_lane(const GnView& v, const int64_t ia, const int64_t ib, const double* x, const long long n,
                                                 const int c, double* var, double* dist) {
    double u[DIM], d[2 * DIM];
    const double rho = lv_pair_direction<DIM>(v, ia, ib, u);
    lv_read<DIM>(x, n, c, lv_point_first<DIM>(v.Np, ia), d);
    lv_read<DIM>(x, n, c, lv_point_first<DIM>(v.Np, ib), d + DIM);
    double y = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) y += u[k] * d[k];
#pragma unroll
    for (int k = 0; k < DIM; ++k) y += -u[k] * d[DIM + k];
    *var = y;
    *dist = rho;
}

// one lane per live pair of the block
template <int DIM>
__global__ __launch_bounds__(64) void k_lv_pair_dot(LvPairArgs a) {
    const int c = threadIdx.x;
    if (c >= a.live) return;
    const long long p = a.c0 + c;
    lv_pair_dot_lane<DIM>(a.v, a.pa[p], a.pb[p], a.x, a.n, c, a.var + p, a.dist + p);
}

// The buffers of both calls: they stay with the refinement handle between calls, as PsWork's do (the pairs' grow on demand).
struct LvWork {
    DevBuf<double> sums, pair_sums, b, var, dist;
    DevBuf<int32_t> pa, pb;
    size_t pair_room = 0;
    void reserve_pairs(int32_t n_pairs) {
        if ((size_t)n_pairs <= pair_room && pa.d) return;
        NoArena no_arena;
        pair_room = (size_t)std::max<int32_t>(16, n_pairs);
        pa.alloc(pair_room); pb.alloc(pair_room); pair_sums.alloc(2 * pair_room); var.alloc(pair_room); dist.alloc(pair_room);
    }
    void send_pairs(const int32_t* a, const int32_t* b, int32_t n_pairs, hipStream_t st) {
        reserve_pairs(n_pairs);
        if (n_pairs > 0) {
            staged_h2d(pa.d, a, (size_t)n_pairs * sizeof(int32_t), st);
            staged_h2d(pb.d, b, (size_t)n_pairs * sizeof(int32_t), st);
        }
    }
};

// the listed pairs are variable ids as in score_graph's range endpoints
inline void lv_check_pairs(const GnProblem& P, const int32_t* pair_a, const int32_t* pair_b, int32_t n_pairs, const std::string& who) {
    if (n_pairs < 0) throw std::runtime_error(who + "n_pairs must be >= 0");
    if (n_pairs > 0 && !(pair_a && pair_b)) throw std::runtime_error(who + "n_pairs pairs without their lists");
    for (int32_t c = 0; c < n_pairs; ++c) {
        const int64_t a = pair_a[c], b = pair_b[c];
        if (a < 0 || a >= P.Np + P.Nl || b < 0 || b >= P.Np + P.Nl) throw std::runtime_error(who + "a pair's variable is out of range");
        if (a == b) throw std::runtime_error(who + "a pair joins a variable to itself");
    }
}


// What score_refine_leverage does with a solved block -- the consumer ps_solve is given (as PsMoments is the samples').
struct LvMeasure {
    const int32_t* pair_a; const int32_t* pair_b; int32_t n_pairs;
    double* lev_sum; double* lev_sq; double* red_sum; double* red_sq; double* pair_sum; double* pair_sq;
    LvArgs l{};
    LvWork* L = nullptr;
    void check(const GnProblem& P, const std::string& who) { lv_check_pairs(P, pair_a, pair_b, n_pairs, who); }
    template <class Refine>
    void begin(Refine& R, PsArgs& q, MvArgs&, hipStream_t st) {
        L = &R.lv;
        const size_t M = (size_t)R.P.n_meas();
        if (!L->sums.d) {
            NoArena no_arena;
            L->sums.alloc(4 * M);
        }
        L->send_pairs(pair_a, pair_b, n_pairs, st);
        L->sums.zero(st); L->pair_sums.zero(st);
        l.v = R.view(R.u.d); l.seed = q.seed; l.x = R.mv.x.d; l.n = R.P.n; l.M = R.P.n_meas();
        l.sums = L->sums.d; l.pa = L->pa.d; l.pb = L->pb.d; l.n_pairs = n_pairs; l.pair_sums = L->pair_sums.d;
    }
    template <class Refine>
    void block(Refine& R, const PsArgs& q, const MvArgs&, int, int live, hipStream_t st) {
        if (!q.take) return;
        l.s0 = q.s0; l.live = live; l.take = q.take;
        const unsigned grid = (unsigned)std::max<long long>(1, (l.M + n_pairs + kThreads - 1) / kThreads);
        gn_dim(R.P.dim, [&](auto dim) { hipLaunchKernelGGL(k_lv_measure<decltype(dim)::value>, dim3(grid), dim3(kThreads), 0, st, l); });
    }
    void end(hipStream_t st) {
        const size_t M = (size_t)l.M, f8 = sizeof(double), np = (size_t)n_pairs;
        double* out[4] = {lev_sum, lev_sq, red_sum, red_sq};
        for (int k = 0; k < 4; ++k)
            if (out[k]) staged_d2h(out[k], L->sums.d + (size_t)k * M, M * f8, st);
        if (pair_sum) staged_d2h(pair_sum, L->pair_sums.d, np * f8, st);
        if (pair_sq) staged_d2h(pair_sq, L->pair_sums.d + np, np * f8, st);
    }
};

// What lv_pair_solve does with a solved block beyond its variance -- the consumer it is given, as ps_solve is given LvMeasure:
// check (the consumer's own arguments, before any work), begin (the block arguments stand), block (after k_lv_pair_dot of the
// block c0 .. c0 + live, its solutions still in the block's x), end (every block solved and read: col_done[c] = 1 where column
// c converged).  score_refine_range_variances has none; score_refine_select_ranges (score_select.hpp) forms the cross terms.
struct LvPairOnly {
    void check(int32_t, const std::string&) {}
    template <class Refine>
    void begin(Refine&, const LvPairArgs&, int32_t, hipStream_t) {}
    template <class Refine>
    void block(Refine&, int, int, hipStream_t) {}
    void end(const std::vector<int32_t>&, hipStream_t) {}
};

// score_refine_range_variances.  Refine: score_refine (its point, blocks and gather, its linear-mode handle, its MvWork and LvWork).
template <class Refine, class Use>
int lv_pair_solve(Refine& R, const std::string& who, const double* poses, const double* landmarks, const int32_t* pair_a,
                  const int32_t* pair_b, int32_t n_pairs, double rel_tol, int32_t max_iters, int32_t block_width, double* variances,
                  double* distances, double* residuals, int32_t* iters, double* solutions, score_marginals_info* info, Use& use) {
    const GnProblem& P = R.P;
    if (block_width < 1 || block_width > kMvMaxWidth) throw std::runtime_error(who + "block_width must be 1..16");
    if (!(rel_tol > 0.0) || max_iters < 1) throw std::runtime_error(who + "rel_tol must be positive and max_iters >= 1");
    lv_check_pairs(P, pair_a, pair_b, n_pairs, who);
    use.check(n_pairs, who);
    HipBackend& be = R.be();
    hipStream_t st = R.stream();
    const long long n = P.n;
    const double t0 = now_ms();
    R.h_at_point(poses, landmarks, who, "blocks of columns need");
    be.derive_rho_data(false);
    const int NV = mv_slots(block_width);
    auto& W = R.mv;
    auto& L = R.lv;
    W.reserve(P, R.product_tiles(), be.n_prec, be.H->bs * be.n_join_seps, st);
    if (!L.b.d) {
        NoArena no_arena;
        L.b.alloc((size_t)kMvMaxWidth * (size_t)n); L.b.zero(st);
    }
    L.send_pairs(pair_a, pair_b, n_pairs, st);
    const int n_rblocks = (int)((n + kMvThreads - 1) / kMvThreads);
    MvArgs a = mv_block_args(be, W, n, rel_tol);
    LvPairArgs l{};
    l.v = R.view(R.u.d); l.x = W.x.d; l.n = n; l.pa = L.pa.d; l.pb = L.pb.d; l.b = L.b.d; l.var = L.var.d; l.dist = L.dist.d;
    use.begin(R, l, n_pairs, st);
    const double t1 = now_ms();
    const size_t C = (size_t)n_pairs;
    std::vector<int32_t> flags((size_t)kMvFlagWords), col_done(C, 0), col_iters(C, 0);
    std::vector<double> res_part((size_t)NV * (size_t)n_rblocks), col_res(C, 0.0);
    int batches = 0, pcg_iters = 0;
    for (int c0 = 0; c0 < n_pairs; c0 += block_width) {
        const int live = std::min<int>(block_width, n_pairs - c0);
        a.c0 = 0; a.live = live;
        l.c0 = c0; l.live = live;
        gn_dim(P.dim, [&](auto dim) {
            hipLaunchKernelGGL(k_lv_pair_rhs<decltype(dim)::value>, dim3((unsigned)n_rblocks, (unsigned)NV), dim3(kMvThreads), 0, st, a, l);
        });
        mv_block_pcg(be, W, a, NV, n_rblocks, max_iters, flags, st);
        // the true residual of every column of the block (one more product, w = H x) against its g, and g'x
        a.all_columns = 1; a.p_in = W.x.d;
        mv_launch_product(a, NV, st);
        hipLaunchKernelGGL(k_ps_residual, dim3((unsigned)n_rblocks, (unsigned)live), dim3(kMvThreads), 0, st, a, (const double*)L.b.d);
        gn_dim(P.dim, [&](auto dim) { hipLaunchKernelGGL(k_lv_pair_dot<decltype(dim)::value>, dim3(1), dim3(64), 0, st, l); });
        use.block(R, c0, live, st);
        HIP_CHECK(hipGetLastError());
        staged_d2h(res_part.data(), W.res_part.d, (size_t)live * (size_t)n_rblocks * sizeof(double), st);
        if (solutions) staged_d2h(solutions + (size_t)c0 * (size_t)n, W.x.d, (size_t)live * (size_t)n * sizeof(double), st);
        int most = 0;
        for (int c = 0; c < live; ++c) {
            double s = 0.0;
            for (int b = 0; b < n_rblocks; ++b) s += res_part[(size_t)c * (size_t)n_rblocks + (size_t)b];
            const double rho = std::sqrt(s);
            col_res[(size_t)(c0 + c)] = rho;
            col_done[(size_t)(c0 + c)] = (flags[(size_t)(kMvDone + c)] == 1 && std::isfinite(rho)) ? 1 : 0;
            col_iters[(size_t)(c0 + c)] = flags[(size_t)(kMvIters + c)];
            most = std::max(most, flags[(size_t)(kMvIters + c)]);
        }
        pcg_iters += most;
        ++batches;
    }
    if (variances) staged_d2h(variances, L.var.d, C * sizeof(double), st);
    if (distances) staged_d2h(distances, L.dist.d, C * sizeof(double), st);
    HIP_CHECK(sync_stream(st));
    const double t2 = now_ms();
    double worst = 0.0;
    const int unconverged = mv_report(col_done, col_iters, col_res, residuals, iters, worst);
    if (info) {
        info->columns = n_pairs; info->batches = batches; info->pcg_iters = pcg_iters; info->unconverged = unconverged;
        info->max_residual = worst; info->setup_ms = t1 - t0; info->solve_ms = t2 - t1;
    }
    use.end(col_done, st);
    return unconverged ? 1 : 0;
}

}  // namespace score

#endif  // __HIPCC__

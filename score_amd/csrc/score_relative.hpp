// score_relative.hpp -- predicted relative poses between listed pairs of poses and their covariances at the refined estimate
// (include/score_relative.h).  For a pair (a, b) the prediction is T_a^-1 T_b = (R_ab, t_ab) = (R_a'R_b, R_a'(t_b - t_a)); with
// G (DP x 2 DP) the derivative of its error coordinates xi in the unknowns of a and b, its covariance is P = G H^-1 G': DP
// columns H x_j = G'e_q of the marginals' lock-step iteration (mv_block_pcg) per pair, where the joint marginal of both ends
// needs 2 DP.
//
// What exists already and is used as it is: the iteration, the product, the residual partials and the tail (mv_block_pcg,
// mv_launch_product, k_ps_residual, mv_report), exactly as lv_pair_solve (score_leverage.hpp) uses them.  New here:
//   rp_pair_jac<DIM>  R_ab, t_ab and G of one pair at the view's point (host and device: tests/tools/relative_jac_check.cpp
//                     compiles this text with g++)
//   k_rp_rhs<DIM>     x = 0, r = b = G_c'e_q for the block's live columns, the done / iteration words as k_lv_pair_rhs sets them
//   k_rp_dot<DIM>     one lane per live column j = c DP + q: P_c[:, q] = G_c x_j from the at most 2 DP entries of x_j at the
//                     pair's unknowns; the lane of q == 0 also writes R_ab and t_ab
// The two kernels' bodies are the device functions rp_rhs_entry and rp_dot_lane on a GnView: the kernels here call them for a
// graph, score_relative_batch.hpp's for a member of a group (the convention of lv_pair_entry / lv_pair_dot_lane).
// Columns, not pairs, fill a block: column j = c DP + q, a block is block_width CONSECUTIVE columns, so a pair may straddle
// two blocks and every slot of a full block is live.  An output entry is formed from its own column alone, in a fixed order,
// without atomics: two calls give the same bits.
//
// Access pattern.  k_rp_rhs is an n x NV streaming store (three arrays, consecutive lanes consecutive rows); only the at most
// 2 DP rows of a column's pair evaluate the Jacobian -- every other thread compares its row with two ranges and stores zeros.
// k_rp_dot reads 2 DP consecutive doubles twice per lane and stores DP entries DP apart: tens of bytes per column.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/score_relative.h"
#include "score_leverage.hpp"

namespace score {

// The pair (a, b) of poses at the view's point: Rab (DIM x DIM, row-major) = R_a'R_b, tab (DIM) = R_a'(t_b - t_a), and
// G (DP x 2 DP, row-major): d xi / d [unknowns of a | unknowns of b] at zero step, xi the error coordinates of the relative
// pose, rotation first -- 2-D (theta_ab + xi_0, t_ab + xi_1:2), 3-D (R_ab Exp(xi_0:2), t_ab + xi_3:5).  With S = [[0, -1], [1, 0]]:
//   2-D  rotation row:     -1 at theta_a, +1 at theta_b
//        translation rows: -S t_ab at theta_a, -R_a' at (x_a, y_a), +R_a' at (x_b, y_b)
//   3-D  rotation rows:    -R_ab' at omega_a, I at omega_b
//        translation rows: [t_ab]x at omega_a, -R_a' at v_a, +R_a' at v_b
// The columns of a pose without unknowns (pose 0) are filled like any other; the callers leave them out.
template <int DIM>
SCORE_GN_HD void rp_pair_jac(const GnView& v, int64_t a, int64_t b, double* Rab, double* tab, double* G) {
    constexpr int DP = DIM == 2 ? 3 : 6, NC = 2 * DP, RO = DP - DIM;  // RO: the first translation unknown of a pose
    double Ra[DIM * DIM], Rb[DIM * DIM], d[DIM];
    if constexpr (DIM == 2) {
        const double* pa = v.X + 3 * a;
        const double* pb = v.X + 3 * b;
        const double ca = cos(pa[0]), sa = sin(pa[0]), cb = cos(pb[0]), sb = sin(pb[0]);
        Ra[0] = ca; Ra[1] = -sa; Ra[2] = sa; Ra[3] = ca;
        Rb[0] = cb; Rb[1] = -sb; Rb[2] = sb; Rb[3] = cb;
        const double* ta = gn_point2(v.X, v.Np, a);
        const double* tb = gn_point2(v.X, v.Np, b);
        d[0] = tb[0] - ta[0]; d[1] = tb[1] - ta[1];
    } else {
        const double* pa = v.X + 12 * a;
        const double* pb = v.X + 12 * b;
#pragma unroll
        for (int k = 0; k < 9; ++k) { Ra[k] = pa[k]; Rb[k] = pb[k]; }
        const double* ta = gn_point3(v.X, v.Np, a);
        const double* tb = gn_point3(v.X, v.Np, b);
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = tb[k] - ta[k];
    }
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < DIM; ++k) t += Ra[k * DIM + i] * d[k];
        tab[i] = t;
#pragma unroll
        for (int j = 0; j < DIM; ++j) {
            double r = 0.0;
#pragma unroll
            for (int k = 0; k < DIM; ++k) r += Ra[k * DIM + i] * Rb[k * DIM + j];
            Rab[i * DIM + j] = r;
        }
    }
#pragma unroll
    for (int k = 0; k < DP * NC; ++k) G[k] = 0.0;
    if constexpr (DIM == 2) {
        G[0] = -1.0; G[DP] = 1.0;
        G[1 * NC] = tab[1]; G[2 * NC] = -tab[0];  // -S t_ab
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = 0; k < 3; ++k) G[i * NC + k] = -Rab[k * 3 + i];
            G[i * NC + DP + i] = 1.0;
        }
        G[3 * NC + 1] = -tab[2]; G[3 * NC + 2] = tab[1];
        G[4 * NC + 0] = tab[2];  G[4 * NC + 2] = -tab[0];
        G[5 * NC + 0] = -tab[1]; G[5 * NC + 1] = tab[0];
    }
#pragma unroll
    for (int i = 0; i < DIM; ++i)
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            G[(RO + i) * NC + RO + k] = -Ra[k * DIM + i];
            G[(RO + i) * NC + DP + RO + k] = Ra[k * DIM + i];
        }
}

}  // namespace score

#if defined(__HIPCC__)

namespace score {

// a block of columns of rp_solve
struct RpArgs {
    GnView v;                    // the graph at the point
    const double* x;             // [c * n + i]: the block's solutions
    long long n;
    const int32_t* pa; const int32_t* pb;
    long long j0;                // the block's first column (column j: pair j / DP, error coordinate j % DP)
    int live;                    // the block's columns
    double* b;                   // [c * n + i]: the right-hand side of the block's column c
    double* cov; double* rot; double* trans;  // per pair: DP x DP, DIM x DIM, DIM
};

// What one thread does for row `row` of the column of error coordinate q of the pair ia - ib of the view: the entry of
// G'e_q there -- stated once for a graph (k_rp_rhs) and for a member of a group (k_grp_rhs, score_relative_batch.hpp).  A row
// that is none of the pair's unknowns is zero and never evaluates the Jacobian; the entry is picked by an unrolled
// compare-select, so G stays in registers.
template <int DIM>
__device__ __forceinline__ double rp_rhs_entry(const GnView& v, const int64_t ia, const int64_t ib, const int q, const long long row) {
    constexpr int DP = DIM == 2 ? 3 : 6, NC = 2 * DP;
    const long long fa = lv_pose_first<DIM>(ia), fb = lv_pose_first<DIM>(ib);
    const bool at_a = fa >= 0 && row >= fa && row < fa + DP, at_b = fb >= 0 && row >= fb && row < fb + DP;
    double g = 0.0;
    if (at_a || at_b) {
        double Rab[DIM * DIM], tab[DIM], G[DP * NC];
        rp_pair_jac<DIM>(v, ia, ib, Rab, tab, G);
        const int col = at_a ? (int)(row - fa) : DP + (int)(row - fb);
#pragma unroll
        for (int qq = 0; qq < DP; ++qq)
#pragma unroll
            for (int k = 0; k < NC; ++k)
                if (qq == q && k == col) g = G[qq * NC + k];
    }
    return g;
}

// grid (row blocks, columns): x = 0, r = b = G_c'e_q of column j0 + c (columns beyond `live`: zero, done from the start)
template <int DIM>
__global__ __launch_bounds__(kMvThreads) void k_rp_rhs(MvArgs m, RpArgs a) {
    constexpr int DP = DIM == 2 ? 3 : 6;
    const int c = blockIdx.y, t = threadIdx.x;
    const long long i = (long long)blockIdx.x * kMvThreads + t;
    const bool on = c < a.live;
    if (i < a.n) {
        double g = 0.0;
        if (on) {
            const long long j = a.j0 + c, p = j / DP;
            g = rp_rhs_entry<DIM>(a.v, a.pa[p], a.pb[p], (int)(j - p * DP), i);
        }
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

// The product of a pair's Jacobian with one solved column -- the body of rp_dot_lane, stated once: y[q'] = sum_k G[q', k] x[k]
// over the unknowns of a, then of b, ascending, from column `slot` of x, stored at P[q' * stride]; Rab, tab: R_ab and t_ab of
// the pair.  rp_dot_lane stores a pair's own DP x DP block (stride DP), k_selp_cross (score_select_poses.hpp) a column of the
// N x N matrix of all candidates (stride N): the same operations in the same order, so the same bits.
template <int DIM>
__device__ __forceinline__ void rp_dot_rows(const GnView& v, const int64_t ia, const int64_t ib, const double* x, const long long n,
                                            const int slot, double* P, const long long stride, double* Rab, double* tab) {
    constexpr int DP = DIM == 2 ? 3 : 6, NC = 2 * DP;
    double G[DP * NC], d[NC];
    rp_pair_jac<DIM>(v, ia, ib, Rab, tab, G);
    lv_read<DP>(x, n, slot, lv_pose_first<DIM>(ia), d);
    lv_read<DP>(x, n, slot, lv_pose_first<DIM>(ib), d + DP);
#pragma unroll
    for (int qq = 0; qq < DP; ++qq) {
        double y = 0.0;
#pragma unroll
        for (int k = 0; k < NC; ++k) y += G[qq * NC + k] * d[k];
        P[qq * stride] = y;
    }
}

// What one lane does for the solved column of error coordinate q of the pair ia - ib, its solution in column `slot` of x:
// P[q' DP] = sum_k G[q', k] x[k] over the unknowns of a, then of b, ascending (P: the pair's block at its column q); the lane
// of q == 0 also writes R_ab and t_ab (rot, trans: the pair's own) -- stated once for a graph and for a group (k_grp_dot).
template <int DIM>
__device__ __forceinline__ void rp_dot_lane(const GnView& v, const int64_t ia, const int64_t ib, const int q, const double* x,
                                            const long long n, const int slot, double* P, double* rot, double* trans) {
    constexpr int DP = DIM == 2 ? 3 : 6;
    double Rab[DIM * DIM], tab[DIM];
    rp_dot_rows<DIM>(v, ia, ib, x, n, slot, P, DP, Rab, tab);
    if (q == 0) {
#pragma unroll
        for (int k = 0; k < DIM * DIM; ++k) rot[k] = Rab[k];
#pragma unroll
        for (int k = 0; k < DIM; ++k) trans[k] = tab[k];
    }
}

// one lane per live column of the block
template <int DIM>
__global__ __launch_bounds__(64) void k_rp_dot(RpArgs a) {
    constexpr int DP = DIM == 2 ? 3 : 6;
    const int c = threadIdx.x;
    if (c >= a.live) return;
    const long long j = a.j0 + c, p = j / DP;
    const int q = (int)(j - p * DP);
    rp_dot_lane<DIM>(a.v, a.pa[p], a.pb[p], q, a.x, a.n, c, a.cov + p * (DP * DP) + q, a.rot + p * (DIM * DIM), a.trans + p * DIM);
}

// The buffers of the call: they stay with the refinement handle between calls, as LvWork's do (the pairs' grow on demand).
struct RpWork {
    DevBuf<double> b, cov, rot, trans;
    DevBuf<int32_t> pa, pb;
    size_t pair_room = 0;
    void send_pairs(const int32_t* a, const int32_t* b_, int32_t n_pairs, int dim, hipStream_t st) {
        if ((size_t)n_pairs > pair_room || !pa.d) {
            NoArena no_arena;
            const size_t dp = dim == 2 ? 3 : 6, d = (size_t)dim;
            pair_room = (size_t)std::max<int32_t>(16, n_pairs);
            pa.alloc(pair_room); pb.alloc(pair_room);
            cov.alloc(pair_room * dp * dp); rot.alloc(pair_room * d * d); trans.alloc(pair_room * d);
        }
        staged_h2d(pa.d, a, (size_t)n_pairs * sizeof(int32_t), st);
        staged_h2d(pb.d, b_, (size_t)n_pairs * sizeof(int32_t), st);
    }
};

// the listed pairs join two different poses (pose 0 included: it has a place and no unknowns)
inline void rp_check_pairs(const GnProblem& P, const int32_t* pair_a, const int32_t* pair_b, int32_t n_pairs, const std::string& who) {
    if (n_pairs < 0) throw std::runtime_error(who + "n_pairs must be >= 0");
    if (n_pairs > 0 && !(pair_a && pair_b)) throw std::runtime_error(who + "n_pairs pairs without their lists");
    if ((long long)n_pairs * 36 > INT32_MAX) throw std::runtime_error(who + "too many pairs for one call");
    for (int32_t c = 0; c < n_pairs; ++c) {
        const int64_t a = pair_a[c], b = pair_b[c];
        if (a < 0 || a >= P.Np || b < 0 || b >= P.Np) throw std::runtime_error(who + "a pair's pose is out of range (a landmark has no relative pose)");
        if (a == b) throw std::runtime_error(who + "a pair joins a pose to itself");
    }
}

// What rp_solve does with a solved block beyond its covariances -- the consumer it is given, as lv_pair_solve is given
// LvPairOnly / SelCross: check (the consumer's own arguments, before any work), begin (the block arguments stand), block (after
// k_rp_dot of the columns j0 .. j0 + live, their solutions still in the block's x), end (every block solved and read:
// col_done[j] = 1 where column j converged).  score_refine_relative_covariances has none;
// score_refine_select_relative_poses (score_select_poses.hpp) forms the cross terms.
struct RpOnly {
    void check(int32_t, const std::string&) {}
    template <class Refine>
    void begin(Refine&, const RpArgs&, int32_t, hipStream_t) {}
    template <class Refine>
    void block(Refine&, long long, int, hipStream_t) {}
    void end(const std::vector<int32_t>&, hipStream_t) {}
};

// score_refine_relative_covariances.  Refine: score_refine (its point, blocks and gather, its linear-mode handle, its MvWork and RpWork).
template <class Refine, class Use>
int rp_solve(Refine& R, const std::string& who, const double* poses, const double* landmarks, const int32_t* pair_a, const int32_t* pair_b,
             int32_t n_pairs, double rel_tol, int32_t max_iters, int32_t block_width, double* rotations, double* translations,
             double* covariances, double* residuals, int32_t* iters, double* solutions, score_marginals_info* info, Use& use) {
    const GnProblem& P = R.P;
    if (block_width < 1 || block_width > kMvMaxWidth) throw std::runtime_error(who + "block_width must be 1..16");
    if (!(rel_tol > 0.0) || max_iters < 1) throw std::runtime_error(who + "rel_tol must be positive and max_iters >= 1");
    rp_check_pairs(P, pair_a, pair_b, n_pairs, who);
    use.check(n_pairs, who);
    if (n_pairs == 0) {
        if (info) *info = score_marginals_info{};
        return 0;
    }
    HipBackend& be = R.be();
    hipStream_t st = R.stream();
    const long long n = P.n;
    const int dim = P.dim, DP = dim == 2 ? 3 : 6;
    const double t0 = now_ms();
    R.h_at_point(poses, landmarks, who, "blocks of columns need");
    be.derive_rho_data(false);
    const int NV = mv_slots(block_width);
    auto& W = R.mv;
    auto& L = R.rp;
    W.reserve(P, R.product_tiles(), be.n_prec, be.H->bs * be.n_join_seps, st);
    if (!L.b.d) {
        NoArena no_arena;
        L.b.alloc((size_t)kMvMaxWidth * (size_t)n); L.b.zero(st);
    }
    L.send_pairs(pair_a, pair_b, n_pairs, dim, st);
    const int n_rblocks = (int)((n + kMvThreads - 1) / kMvThreads);
    MvArgs a = mv_block_args(be, W, n, rel_tol);
    RpArgs l{};
    l.v = R.view(R.u.d); l.x = W.x.d; l.n = n; l.pa = L.pa.d; l.pb = L.pb.d; l.b = L.b.d;
    l.cov = L.cov.d; l.rot = L.rot.d; l.trans = L.trans.d;
    use.begin(R, l, n_pairs, st);
    const double t1 = now_ms();
    const long long columns = (long long)n_pairs * DP;
    const size_t C = (size_t)columns;
    std::vector<int32_t> flags((size_t)kMvFlagWords), col_done(C, 0), col_iters(C, 0);
    std::vector<double> res_part((size_t)NV * (size_t)n_rblocks), col_res(C, 0.0);
    int batches = 0, pcg_iters = 0;
    for (long long j0 = 0; j0 < columns; j0 += block_width) {
        const int live = (int)std::min<long long>(block_width, columns - j0);
        a.c0 = 0; a.live = live;
        l.j0 = j0; l.live = live;
        gn_dim(dim, [&](auto d) {
            hipLaunchKernelGGL(k_rp_rhs<decltype(d)::value>, dim3((unsigned)n_rblocks, (unsigned)NV), dim3(kMvThreads), 0, st, a, l);
        });
        mv_block_pcg(be, W, a, NV, n_rblocks, max_iters, flags, st);
        // the true residual of every column of the block (one more product, w = H x) against its right-hand side, and G x
        a.all_columns = 1; a.p_in = W.x.d;
        mv_launch_product(a, NV, st);
        hipLaunchKernelGGL(k_ps_residual, dim3((unsigned)n_rblocks, (unsigned)live), dim3(kMvThreads), 0, st, a, (const double*)L.b.d);
        gn_dim(dim, [&](auto d) { hipLaunchKernelGGL(k_rp_dot<decltype(d)::value>, dim3(1), dim3(64), 0, st, l); });
        use.block(R, j0, live, st);
        HIP_CHECK(hipGetLastError());
        staged_d2h(res_part.data(), W.res_part.d, (size_t)live * (size_t)n_rblocks * sizeof(double), st);
        if (solutions) staged_d2h(solutions + (size_t)j0 * (size_t)n, W.x.d, (size_t)live * (size_t)n * sizeof(double), st);
        int most = 0;
        for (int c = 0; c < live; ++c) {
            double s = 0.0;
            for (int b = 0; b < n_rblocks; ++b) s += res_part[(size_t)c * (size_t)n_rblocks + (size_t)b];
            const double rho = std::sqrt(s);
            col_res[(size_t)(j0 + c)] = rho;
            col_done[(size_t)(j0 + c)] = (flags[(size_t)(kMvDone + c)] == 1 && std::isfinite(rho)) ? 1 : 0;
            col_iters[(size_t)(j0 + c)] = flags[(size_t)(kMvIters + c)];
            most = std::max(most, flags[(size_t)(kMvIters + c)]);
        }
        pcg_iters += most;
        ++batches;
    }
    const size_t np = (size_t)n_pairs, d = (size_t)dim, f8 = sizeof(double);
    if (covariances) staged_d2h(covariances, L.cov.d, np * (size_t)(DP * DP) * f8, st);
    if (rotations) staged_d2h(rotations, L.rot.d, np * d * d * f8, st);
    if (translations) staged_d2h(translations, L.trans.d, np * d * f8, st);
    HIP_CHECK(sync_stream(st));
    const double t2 = now_ms();
    double worst = 0.0;
    const int unconverged = mv_report(col_done, col_iters, col_res, residuals, iters, worst);
    if (info) {
        info->columns = (int32_t)columns; info->batches = batches; info->pcg_iters = pcg_iters; info->unconverged = unconverged;
        info->max_residual = worst; info->setup_ms = t1 - t0; info->solve_ms = t2 - t1;
    }
    use.end(col_done, st);
    return unconverged ? 1 : 0;
}

}  // namespace score

#endif  // __HIPCC__

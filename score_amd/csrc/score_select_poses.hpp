// score_select_poses.hpp -- greedy selection of candidate loop closures by joint information gain
// (include/score_select_poses.h) on the device: the block form of score_select.hpp.  A candidate is a relative pose, a block
// of DP = 3 or 6 columns; the pivot is its DP x DP Schur block, scored by 1/2 logdet.
//
// What exists already and is used as it is: the columns H x = G_c'e_q of rp_solve (score_relative.hpp), which takes the
// consumer of a solved block defined here (SelpCross) the way lv_pair_solve takes SelCross; the product of a pair's Jacobian
// with a solved column (rp_dot_rows: the body of rp_dot_lane with the row stride as an argument, so a diagonal block of P is
// the covariance of k_rp_dot bit for bit); k_sel_sym on the N = C DP columns with their precisions; SelWork's P, L, w, part
// and exclusions; the rule (score_select_poses_rule.hpp: selp_gain, sel_better, selp_stop, selp_scaled, selp_check).  New here:
//   k_selp_cross<DIM>  after each solved block, grid (ceil(C / kThreads), live): the lane of candidate c for column slot s
//                      writes the DP entries P[(c DP + q') N + j0 + s] = (G_c x_s)[q'] -- column j of P is "as computed".
//                      Columns, not candidates, fill a block: a candidate may straddle two blocks.
//   k_selp_greedy<DP>  the whole block-pivoted factorisation in ONE launch of ONE workgroup of kThreads lanes.  Lane t owns
//                      the candidates t + kThreads m.  The blocks B_c live in a global work buffer, entry-major
//                      (Bw[e C + c]: consecutive lanes, consecutive addresses) -- at the caps they take 114 KB, more than a
//                      workgroup's LDS.  LDS holds the DP rows of L at the pivot's columns (12 KB at the caps), the next
//                      sub-step's pivot, the candidates' states and the argmax scratch.  Per step: every lane scores its
//                      eligible candidates (selp_gain), the argmax is a wavefront reduction and a pass over the waves'
//                      results carrying (value, index); then DP sub-steps, each one coalesced sweep over the J columns of L
//                      for the lane's rows, the update of the lane's blocks, and ONE workgroup barrier: the owner of the
//                      pivot appends its DP entries of the new column to the rows in LDS and publishes the next pivot.
// fp64, no atomics, fixed-order sums: two calls give the same bits.  One workgroup is the decision of score_select.hpp: at the
// caps the multiply-add count is the scalar kernel's, N K^2 / 2 with N = 4096 columns and K = 256 columns of L.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/score_select_poses.h"
#include "score_relative.hpp"
#include "score_select.hpp"
#include "score_select_poses_rule.hpp"

#if defined(__HIPCC__)

namespace score {

struct SelpCrossArgs {
    GnView v;                  // the graph at the point
    const double* x;           // [s * n + i]: the block's solutions
    long long n;
    const int32_t* pa; const int32_t* pb;
    int C;                     // candidates
    long long N, j0;           // columns of P, the block's first
    double* P;                 // [r * N + j]
};

// grid (ceil(C / kThreads), live): lane c of column slot s
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_selp_cross(SelpCrossArgs a) {
    constexpr int DP = DIM == 2 ? 3 : 6;
    const int c = (int)blockIdx.x * kThreads + (int)threadIdx.x, s = blockIdx.y;
    if (c >= a.C) return;
    double Rab[DIM * DIM], tab[DIM];
    rp_dot_rows<DIM>(a.v, a.pa[c], a.pb[c], a.x, a.n, s, a.P + (size_t)c * DP * (size_t)a.N + (size_t)(a.j0 + s), a.N, Rab, tab);
}

struct SelpGreedyArgs {
    const double* A;           // [r * N + i], symmetric
    const double* w;           // N: the columns' precisions
    const int32_t* excluded;   // C; non-zero: never picked (null: none)
    int C, k;
    double min_gain;
    double* L;                 // [J * N + i]
    double* Bw;                // [e * C + c]: entry e = q DP + q' of B_c
    int32_t* order; double* gains;   // k each
    double* pick_cov;          // k DP^2
    double* remaining;         // C DP^2
    int32_t* picked;           // 1
};

// ONE workgroup: <<<1, kThreads>>>
template <int DP>
__global__ __launch_bounds__(kThreads) void k_selp_greedy(SelpGreedyArgs a) {
    constexpr int BB = DP * DP, MAXC = selp_max_candidates(DP), OWN = (MAXC + kThreads - 1) / kThreads;
    __shared__ double rows[DP][kSelMaxPicks];   // rows[q][m] = L[p DP + q, m] of the step's pivot p
    __shared__ double piv[DP];                  // piv[q]: B_p[q, q] as the q earlier sub-steps left it
    __shared__ unsigned char state[MAXC];
    __shared__ double best_g[kSelWaves];
    __shared__ int32_t best_i[kSelWaves];
    const int t = threadIdx.x, C = a.C;
    const size_t N = (size_t)C * DP;
    for (int c = t; c < C; c += kThreads) {
#pragma unroll
        for (int e = 0; e < BB; ++e) a.Bw[(size_t)e * C + c] = a.A[((size_t)c * DP + e / DP) * N + (size_t)c * DP + e % DP];
        state[c] = (unsigned char)((a.excluded && a.excluded[c]) ? kSelExcluded : kSelEligible);
    }
    __syncthreads();
    int j = 0;
    for (; j < a.k; ++j) {
        // the lane's best (ascending c: ties to the lowest index), the wave's, the workgroup's
        double bg = 0.0;
        int32_t bi = -1;
        for (int c = t; c < C; c += kThreads) {
            if (state[c] != kSelEligible) continue;
            double B[BB];
#pragma unroll
            for (int e = 0; e < BB; ++e) B[e] = a.Bw[(size_t)e * C + c];
            const double g = selp_gain<DP>(B);
            if (sel_better(g, c, bg, bi)) { bg = g; bi = c; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double og = __shfl_down(bg, off, 64);
            const int32_t oi = __shfl_down(bi, off, 64);
            if (sel_better(og, oi, bg, bi)) { bg = og; bi = oi; }
        }
        if ((t & 63) == 0) { best_g[t / 64] = bg; best_i[t / 64] = bi; }
        __syncthreads();
        double gp = best_g[0];
        int32_t p = best_i[0];
        for (int q = 1; q < kSelWaves; ++q)
            if (sel_better(best_g[q], best_i[q], gp, p)) { gp = best_g[q]; p = best_i[q]; }
        if (p < 0 || selp_stop(gp, a.min_gain)) break;   // (the same p and gain in every lane: the workgroup leaves together)
        const int JJ = j * DP;
        for (int i = t; i < DP * JJ; i += kThreads) rows[i / JJ][i % JJ] = a.L[(size_t)(i % JJ) * N + (size_t)p * DP + i / JJ];
        if (t == p % kThreads) {   // the owner of p: the record, before its block moves
            double B[BB], wp[DP];
#pragma unroll
            for (int e = 0; e < BB; ++e) B[e] = a.Bw[(size_t)e * C + p];
#pragma unroll
            for (int q = 0; q < DP; ++q) wp[q] = a.w[(size_t)p * DP + q];
#pragma unroll
            for (int e = 0; e < BB; ++e) {
                const double v = selp_scaled<DP>(B, wp, e / DP, e % DP);
                a.pick_cov[(size_t)j * BB + e] = v;
                a.remaining[(size_t)p * BB + e] = v;
            }
            a.order[j] = p; a.gains[j] = gp;
            state[p] = (unsigned char)kSelPicked;
            piv[0] = B[0];
        }
        __syncthreads();
        for (int q = 0; q < DP; ++q) {
            const int J = JJ + q;
            const size_t r = (size_t)p * DP + q;
            // l_i for the rows of the lane's candidates: row r of A, then the J columns of L in ascending order
            double acc[OWN][DP];
#pragma unroll
            for (int m = 0; m < OWN; ++m) {
                const int c = t + kThreads * m;
#pragma unroll
                for (int e = 0; e < DP; ++e) acc[m][e] = c < C ? a.A[r * N + (size_t)c * DP + e] : 0.0;
            }
            for (int i = 0; i < J; ++i) {
                const double lp = rows[q][i];
                const double* Li = a.L + (size_t)i * N;
#pragma unroll
                for (int m = 0; m < OWN; ++m) {
                    const int c = t + kThreads * m;
                    if (c < C) {
#pragma unroll
                        for (int e = 0; e < DP; ++e) acc[m][e] -= Li[(size_t)c * DP + e] * lp;
                    }
                }
            }
            const double root = sqrt(piv[q]);
#pragma unroll
            for (int m = 0; m < OWN; ++m) {
                const int c = t + kThreads * m;
                if (c < C) {
                    double l[DP];
#pragma unroll
                    for (int e = 0; e < DP; ++e) {
                        l[e] = acc[m][e] / root;
                        a.L[(size_t)J * N + (size_t)c * DP + e] = l[e];
                    }
#pragma unroll
                    for (int e = 0; e < BB; ++e) {   // (the lower triangle, mirrored: the blocks stay symmetric bit for bit)
                        if (e / DP < e % DP) continue;
                        const double b = a.Bw[(size_t)e * C + c] - l[e / DP] * l[e % DP];
                        a.Bw[(size_t)e * C + c] = b;
                        if (e / DP != e % DP) a.Bw[(size_t)((e % DP) * DP + e / DP) * C + c] = b;
                        if (c == p && q + 1 < DP && e == (q + 1) * (DP + 1)) piv[q + 1] = b;
                    }
                    if (c == p) {
#pragma unroll
                        for (int e = 0; e < DP; ++e) rows[e][J] = l[e];
                    }
                }
            }
            __syncthreads();   // (column J of L, the pivot's rows of it, the next pivot and the blocks are the next sub-step's)
        }
    }
    for (int i = j + t; i < a.k; i += kThreads) { a.order[i] = -1; a.gains[i] = 0.0; }
    for (int i = j * BB + t; i < a.k * BB; i += kThreads) a.pick_cov[i] = 0.0;
    for (int c = t; c < C; c += kThreads) {
        if (state[c] == kSelPicked) continue;
        double B[BB], wc[DP];
#pragma unroll
        for (int e = 0; e < BB; ++e) B[e] = a.Bw[(size_t)e * C + c];
#pragma unroll
        for (int q = 0; q < DP; ++q) wc[q] = a.w[(size_t)c * DP + q];
#pragma unroll
        for (int e = 0; e < BB; ++e) a.remaining[(size_t)c * BB + e] = selp_scaled<DP>(B, wc, e / DP, e % DP);
    }
    if (t == 0) *a.picked = j;
}

// What the blocks need beside SelWork's P / L / w / part / excluded / order / gains / picked: they stay with the refinement
// handle between calls too.
struct SelpWork {
    DevBuf<double> Bw, pick_cov, remaining;
    size_t room = 0;
    void reserve(int32_t C, int DP) {
        NoArena no_arena;
        const size_t need = (size_t)C * (size_t)(DP * DP);
        if (need > room || !Bw.d) {
            room = need;
            Bw.alloc(room); remaining.alloc(room);
        }
        if (!pick_cov.d) pick_cov.alloc((size_t)kSelMaxPicks * 6);   // k DP^2 <= (256 / DP) DP^2
    }
};

struct SelpOutputs {
    int32_t* order; double* gains; double* pick_covariances; double* remaining;
};

// the columns' precisions on the device, k_sel_sym and k_selp_greedy on W.P (N x N as computed) and the host's exclusions;
// returns the picks; *asymmetry and *total_gain as score_select_poses_info has them
inline int32_t selp_run(SelWork& W, SelpWork& B, int32_t C, int dim, int32_t k, double min_gain, const double* kappa, const double* tau,
                        const int32_t* excluded, const SelpOutputs& out, double* asymmetry, double* total_gain, hipStream_t st) {
    const int DP = selp_dp(dim), N = C * DP, BB = DP * DP;
    const int T = (N + kSelTile - 1) / kSelTile, pairs = T * (T + 1) / 2;
    std::vector<double> w((size_t)N);
    selp_weights(C, dim, kappa, tau, w.data());
    staged_h2d(W.w.d, w.data(), (size_t)N * sizeof(double), st);
    if (excluded) staged_h2d(W.excluded.d, excluded, (size_t)C * sizeof(int32_t), st);
    hipLaunchKernelGGL(k_sel_sym, dim3((unsigned)pairs), dim3(kThreads), 0, st, W.P.d, (const double*)W.w.d, N, T, W.part.d);
    SelpGreedyArgs g{};
    g.A = W.P.d; g.w = W.w.d; g.excluded = excluded ? W.excluded.d : nullptr; g.C = C; g.k = k; g.min_gain = min_gain;
    g.L = W.L.d; g.Bw = B.Bw.d; g.order = W.order.d; g.gains = W.gains.d; g.pick_cov = B.pick_cov.d; g.remaining = B.remaining.d;
    g.picked = W.picked.d;
    if (dim == 2) hipLaunchKernelGGL(k_selp_greedy<3>, dim3(1), dim3(kThreads), 0, st, g);
    else hipLaunchKernelGGL(k_selp_greedy<6>, dim3(1), dim3(kThreads), 0, st, g);
    HIP_CHECK(hipGetLastError());
    std::vector<double> part((size_t)pairs), gains((size_t)k);
    int32_t picked = 0;
    staged_d2h(part.data(), W.part.d, (size_t)pairs * sizeof(double), st);
    staged_d2h(gains.data(), W.gains.d, (size_t)k * sizeof(double), st);
    staged_d2h(&picked, W.picked.d, sizeof(int32_t), st);
    if (out.order) staged_d2h(out.order, W.order.d, (size_t)k * sizeof(int32_t), st);
    if (out.pick_covariances) staged_d2h(out.pick_covariances, B.pick_cov.d, (size_t)k * BB * sizeof(double), st);
    if (out.remaining) staged_d2h(out.remaining, B.remaining.d, (size_t)C * BB * sizeof(double), st);
    HIP_CHECK(sync_stream(st));
    double worst = 0.0, total = 0.0;
    for (int b = 0; b < pairs; ++b)
        if (part[(size_t)b] > worst) worst = part[(size_t)b];
    for (int32_t j = 0; j < picked; ++j) total += gains[(size_t)j];
    if (out.gains) std::copy(gains.begin(), gains.end(), out.gains);
    if (asymmetry) *asymmetry = worst;
    if (total_gain) *total_gain = total;
    return picked;
}

// What score_refine_select_relative_poses does with a solved block of rp_solve, and with all of them.
struct SelpCross {
    const double* kappa; const double* tau; int32_t k; double min_gain;
    SelpOutputs out; double* matrix; score_select_poses_info* info;
    int dim = 0;
    SelWork* W = nullptr;
    SelpWork* B = nullptr;
    SelpCrossArgs a{};
    bool pending = false;
    double cross_ms = 0.0;
    void settle() {   // (the block's own read of its residuals has waited for the stream)
        if (!pending) return;
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, W->ev0, W->ev1));
        cross_ms += ms;
        pending = false;
    }
    void check(int32_t n_pairs, const std::string& who) { selp_check(n_pairs, dim, k, min_gain, kappa, tau, who); }
    template <class Refine>
    void begin(Refine& R, const RpArgs& l, int32_t n_pairs, hipStream_t) {
        const int DP = selp_dp(dim);
        W = &R.sel;
        B = &R.selp;
        W->reserve(n_pairs * DP, k * DP);
        B->reserve(n_pairs, DP);
        if (!W->ev0) { HIP_CHECK(hipEventCreate(&W->ev0)); HIP_CHECK(hipEventCreate(&W->ev1)); }
        a.v = l.v; a.x = l.x; a.n = l.n; a.pa = l.pa; a.pb = l.pb; a.C = n_pairs; a.N = (long long)n_pairs * DP; a.P = W->P.d;
    }
    template <class Refine>
    void block(Refine& R, long long j0, int live, hipStream_t st) {
        settle();
        a.j0 = j0;
        HIP_CHECK(hipEventRecord(W->ev0, st));
        gn_dim(R.P.dim, [&](auto d) {
            hipLaunchKernelGGL(k_selp_cross<decltype(d)::value>, dim3((unsigned)((a.C + kThreads - 1) / kThreads), (unsigned)live),
                               dim3(kThreads), 0, st, a);
        });
        HIP_CHECK(hipEventRecord(W->ev1, st));
        pending = true;
    }
    // col_done: 1 where the column converged; a candidate with any other column is excluded
    void end(const std::vector<int32_t>& col_done, hipStream_t st) {
        settle();
        const int32_t C = a.C;
        const int DP = selp_dp(dim);
        const double t0 = now_ms();
        if (matrix) staged_d2h(matrix, W->P.d, (size_t)a.N * (size_t)a.N * sizeof(double), st);
        std::vector<int32_t> excluded((size_t)C, 0);
        int32_t n_excluded = 0;
        for (int32_t c = 0; c < C; ++c) {
            for (int q = 0; q < DP; ++q)
                if (!col_done[(size_t)c * DP + q]) excluded[(size_t)c] = 1;
            n_excluded += excluded[(size_t)c];
        }
        double asymmetry = 0.0, total = 0.0;
        const int32_t picked = selp_run(*W, *B, C, dim, k, min_gain, kappa, tau, n_excluded ? excluded.data() : nullptr, out, &asymmetry,
                                        &total, st);
        if (info) {
            info->candidates = C; info->picked = picked; info->excluded = n_excluded; info->total_gain = total;
            info->asymmetry = asymmetry; info->cross_ms = cross_ms; info->greedy_ms = now_ms() - t0;
        }
    }
};

// score_select_block_greedy: the selection on a caller's matrix, buffers of its own
inline void selp_greedy_alone(const double* matrix, const double* kappa, const double* tau, const int32_t* excluded, int32_t C, int32_t dim,
                              int32_t k, double min_gain, const SelpOutputs& out, int32_t* picked, double* asymmetry) {
    const std::string who = "score_select_block_greedy: ";
    selp_check(C, dim, k, min_gain, kappa, tau, who);
    if (!matrix) throw std::runtime_error(who + "the matrix is missing");
    hipStream_t st = nullptr;
    const int DP = selp_dp(dim);
    const size_t N = (size_t)C * DP;
    SelWork W;
    SelpWork B;
    W.reserve((int32_t)N, k * DP);
    B.reserve(C, DP);
    staged_h2d(W.P.d, matrix, N * N * sizeof(double), st);
    const int32_t got = selp_run(W, B, C, dim, k, min_gain, kappa, tau, excluded, out, asymmetry, nullptr, st);
    if (picked) *picked = got;
}

}  // namespace score

#endif  // __HIPCC__

// score_select.hpp -- greedy selection of candidate ranges by joint information gain (include/score_select.h) on the device.
//
// What exists already and is used as it is: the columns x_c = H^-1 g_c of lv_pair_solve (score_leverage.hpp), which takes the
// consumer of a solved block defined here (SelCross) the way ps_solve takes LvMeasure; the gradient of a hypothetical range and
// the entry layout of its dot product (lv_pair_direction through lv_pair_dot_lane: a diagonal entry of P is the variance of
// k_lv_pair_dot bit for bit); the rule (score_select_rule.hpp: sel_better, sel_stop, sel_check).  New here:
//   k_sel_cross<DIM>  after each solved block, grid (ceil(C / kThreads), live): the lane of candidate c writes
//                     P[c C + c0 + s] = g_c'x_s from its at most 2 DIM entries -- column d of P is "as computed"
//   k_sel_sym         A = I + D (P + P')/2 D in place, D = diag(sqrt w), through 32 x 33 LDS tiles, the tile pair (i, j), (j, i)
//                     per workgroup; an entry is formed once per unordered pair of indices, (sqrt w_lo * s) * sqrt w_hi, so A is
//                     symmetric bit for bit; per-workgroup partials of max |P_cd - P_dc|, folded by the host in workgroup order
//   k_sel_greedy      the whole pivoted factorisation in ONE launch of ONE workgroup of kThreads lanes: d, the candidates'
//                     states, the pivot's row L_p,0..j-1 and the reduction scratch in LDS (under 40 KB at the caps), L
//                     (C x k, column j at j C) in global memory; per step one coalesced read of row p of A and of the j
//                     columns of L; the argmax is a wavefront reduction, then a pass over the waves' results in LDS, carrying
//                     (value, index) so that the tie rule is exact
// fp64, no atomics, fixed-order sums: two calls give the same bits.  One workgroup for the factorisation is a decision:
// C k^2 / 2 = 1.3e8 fused multiply-adds at the caps stand next to C / 16 = 256 block solves (profiles/selection.md holds the
// measurement).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/score_select.h"
#include "score_leverage.hpp"
#include "score_select_rule.hpp"

#if defined(__HIPCC__)

namespace score {

constexpr int kSelTile = 32;                                   // the transpose's tile; rows of kSelTile + 1 in LDS
constexpr int kSelOwn = kSelMaxCandidates / kThreads;          // candidates of one lane of k_sel_greedy: c = t + kThreads m
constexpr int kSelWaves = kThreads / 64;

struct SelCrossArgs {
    GnView v;                  // the graph at the point
    const double* x;           // [s * n + i]: the block's solutions
    long long n;
    const int32_t* pa; const int32_t* pb;
    int C, c0;                 // candidates, the block's first
    double* P;                 // [c * C + d]
};

// grid (ceil(C / kThreads), live): lane c of column s
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_sel_cross(SelCrossArgs a) {
    const int c = (int)blockIdx.x * kThreads + (int)threadIdx.x, s = blockIdx.y;
    if (c >= a.C) return;
    double rho;
    lv_pair_dot_lane<DIM>(a.v, a.pa[c], a.pb[c], a.x, a.n, s, a.P + (size_t)c * a.C + a.c0 + s, &rho);
}

// the tile pair of workgroup b among the T (T + 1) / 2 pairs i <= j, row by row
__device__ __forceinline__ void sel_tile_pair(int b, int T, int& i, int& j) {
    i = 0;
    while (b >= T - i) { b -= T - i; ++i; }
    j = i + b;
}
// entry (r, c) of A from p = P_rc and q = P_cr
__device__ __forceinline__ double sel_entry(double p, double q, int r, int c, const double* w) {
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    const double s = 0.5 * (p + q);
    const double v = (sqrt(w[lo]) * s) * sqrt(w[hi]);
    return r == c ? 1.0 + v : v;
}

// What one workgroup does for the tile pair (ti, tj), (tj, ti), ti <= tj, of the C x C matrix P with the precisions w -- stated
// once for a graph (k_sel_sym) and for a member of a group (k_gbsel_sym of score_select_batch.hpp).  kThreads = kSelTile x 8
// lanes, lane (tx, ty) takes the rows ty + 8 q; *part: the workgroup's max |P_cd - P_dc|.
__device__ __forceinline__ void sel_sym_tile_pair(double* P, const double* w, const int C, const int ti, const int tj, double* part) {
    __shared__ double ta[kSelTile][kSelTile + 1], tb[kSelTile][kSelTile + 1];
    __shared__ double wave_max[kSelWaves];
    const int tx = threadIdx.x % kSelTile, ty = threadIdx.x / kSelTile;
    const int r0 = ti * kSelTile, c0 = tj * kSelTile;
    for (int rr = ty; rr < kSelTile; rr += kThreads / kSelTile) {
        const bool in_a = r0 + rr < C && c0 + tx < C, in_b = c0 + rr < C && r0 + tx < C;
        ta[rr][tx] = in_a ? P[(size_t)(r0 + rr) * C + c0 + tx] : 0.0;
        tb[rr][tx] = in_b ? P[(size_t)(c0 + rr) * C + r0 + tx] : 0.0;
    }
    __syncthreads();
    double worst = 0.0;
    for (int rr = ty; rr < kSelTile; rr += kThreads / kSelTile) {
        // tile (i, j): row r0 + rr, column c0 + tx
        if (r0 + rr < C && c0 + tx < C) {
            const double p = ta[rr][tx], q = tb[tx][rr], gap = fabs(p - q);
            if (gap > worst) worst = gap;
            P[(size_t)(r0 + rr) * C + c0 + tx] = sel_entry(p, q, r0 + rr, c0 + tx, w);
        }
        // tile (j, i): row c0 + rr, column r0 + tx
        if (ti != tj && c0 + rr < C && r0 + tx < C)
            P[(size_t)(c0 + rr) * C + r0 + tx] = sel_entry(tb[rr][tx], ta[tx][rr], c0 + rr, r0 + tx, w);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(worst, off, 64);
        if (o > worst) worst = o;
    }
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x / 64] = worst;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = wave_max[0];
        for (int k = 1; k < kSelWaves; ++k)
            if (wave_max[k] > m) m = wave_max[k];
        *part = m;
    }
}

// one workgroup per tile pair (i, j), (j, i), i <= j
__global__ __launch_bounds__(kThreads) void k_sel_sym(double* P, const double* w, int C, int T, double* part) {
    int ti, tj;
    sel_tile_pair((int)blockIdx.x, T, ti, tj);
    sel_sym_tile_pair(P, w, C, ti, tj, part + blockIdx.x);
}

struct SelGreedyArgs {
    const double* A;           // [p * C + c], symmetric
    const double* w;           // precisions
    const int32_t* excluded;   // non-zero: never picked (null: none)
    int C, k;
    double min_gain;
    double* L;                 // [j * C + c]
    int32_t* order; double* gains; double* pick_var;   // k each
    double* remaining;         // C
    int32_t* picked;           // 1
};

// The whole factorisation by ONE workgroup of kThreads lanes -- stated once for a graph (k_sel_greedy) and for a member of a
// group (k_gbsel_greedy of score_select_batch.hpp).  Lane t owns the candidates t + kThreads m, m < kSelOwn.
__device__ __forceinline__ void sel_greedy_workgroup(const SelGreedyArgs& a) {
    __shared__ double d[kSelMaxCandidates];
    __shared__ unsigned char state[kSelMaxCandidates];
    __shared__ double row_p[kSelMaxPicks];
    __shared__ double best_d[kSelWaves];
    __shared__ int32_t best_i[kSelWaves];
    const int t = threadIdx.x, C = a.C;
    for (int c = t; c < C; c += kThreads) {
        d[c] = a.A[(size_t)c * C + c];
        state[c] = (unsigned char)((a.excluded && a.excluded[c]) ? kSelExcluded : kSelEligible);
    }
    __syncthreads();
    int j = 0;
    for (; j < a.k; ++j) {
        // the lane's best (ascending c: ties to the lowest index), the wave's, the workgroup's
        double bd = 0.0;
        int32_t bi = -1;
        for (int c = t; c < C; c += kThreads)
            if (state[c] == kSelEligible && sel_better(d[c], c, bd, bi)) { bd = d[c]; bi = c; }
        for (int off = 32; off > 0; off >>= 1) {
            const double od = __shfl_down(bd, off, 64);
            const int32_t oi = __shfl_down(bi, off, 64);
            if (sel_better(od, oi, bd, bi)) { bd = od; bi = oi; }
        }
        if ((t & 63) == 0) { best_d[t / 64] = bd; best_i[t / 64] = bi; }
        __syncthreads();
        double dp = best_d[0];
        int32_t p = best_i[0];
        for (int q = 1; q < kSelWaves; ++q)
            if (sel_better(best_d[q], best_i[q], dp, p)) { dp = best_d[q]; p = best_i[q]; }
        double gain = 0.0;
        if (p < 0 || sel_stop(dp, a.min_gain, &gain)) break;   // (the same p and d_p in every lane: the workgroup leaves together)
        if (t < j) row_p[t] = a.L[(size_t)t * C + p];
        if (t == 0) {
            const double var = (dp - 1.0) / a.w[p];
            a.order[j] = p; a.gains[j] = gain; a.pick_var[j] = var;
            a.remaining[p] = var;
            state[p] = (unsigned char)kSelPicked;
        }
        __syncthreads();
        // l_c for the lane's candidates: row p of A, then the j columns of L in ascending order
        double acc[kSelOwn];
#pragma unroll
        for (int m = 0; m < kSelOwn; ++m) {
            const int c = t + kThreads * m;
            acc[m] = c < C ? a.A[(size_t)p * C + c] : 0.0;
        }
        for (int i = 0; i < j; ++i) {
            const double lp = row_p[i];
            const double* Li = a.L + (size_t)i * C;
#pragma unroll
            for (int m = 0; m < kSelOwn; ++m) {
                const int c = t + kThreads * m;
                if (c < C) acc[m] -= Li[c] * lp;
            }
        }
        const double root = sqrt(dp);
#pragma unroll
        for (int m = 0; m < kSelOwn; ++m) {
            const int c = t + kThreads * m;
            if (c < C) {
                const double l = acc[m] / root;
                a.L[(size_t)j * C + c] = l;
                d[c] -= l * l;
            }
        }
        __syncthreads();   // (column j of L and d are the next step's)
    }
    for (int i = j + t; i < a.k; i += kThreads) { a.order[i] = -1; a.gains[i] = 0.0; a.pick_var[i] = 0.0; }
    for (int c = t; c < C; c += kThreads)
        if (state[c] != kSelPicked) a.remaining[c] = (d[c] - 1.0) / a.w[c];
    if (t == 0) *a.picked = j;
}

// ONE workgroup: <<<1, kThreads>>>
__global__ __launch_bounds__(kThreads) void k_sel_greedy(SelGreedyArgs a) { sel_greedy_workgroup(a); }

// The buffers of the selection: they stay with the refinement handle between calls, as LvWork's do, and come with the first
// call (P and L grow on demand).
struct SelWork {
    DevBuf<double> P, L, w, gains, pick_var, remaining, part;
    DevBuf<int32_t> excluded, order, picked;
    size_t room = 0, l_room = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void reserve(int32_t C, int32_t k) {
        NoArena no_arena;
        if ((size_t)C > room || !P.d) {
            room = (size_t)C;
            const size_t T = (room + kSelTile - 1) / kSelTile;
            P.alloc(room * room); w.alloc(room); remaining.alloc(room); excluded.alloc(room); part.alloc(T * (T + 1) / 2);
            l_room = 0;
        }
        if ((size_t)C * (size_t)k > l_room || !L.d) {
            l_room = room * (size_t)k;
            L.alloc(l_room);
        }
        if (!order.d) { order.alloc(kSelMaxPicks); gains.alloc(kSelMaxPicks); pick_var.alloc(kSelMaxPicks); picked.alloc(1); }
    }
    ~SelWork() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

struct SelOutputs {
    int32_t* order; double* gains; double* pick_variances; double* remaining;
};

// k_sel_sym and k_sel_greedy on W.P (C x C as computed), W.w and the host's exclusions; returns the picks; *asymmetry and
// *total_gain as score_select_info has them
inline int32_t sel_run(SelWork& W, int32_t C, int32_t k, double min_gain, const int32_t* excluded, const SelOutputs& out,
                       double* asymmetry, double* total_gain, hipStream_t st) {
    const int T = (C + kSelTile - 1) / kSelTile, pairs = T * (T + 1) / 2;
    if (excluded) staged_h2d(W.excluded.d, excluded, (size_t)C * sizeof(int32_t), st);
    hipLaunchKernelGGL(k_sel_sym, dim3((unsigned)pairs), dim3(kThreads), 0, st, W.P.d, (const double*)W.w.d, (int)C, T, W.part.d);
    SelGreedyArgs g{};
    g.A = W.P.d; g.w = W.w.d; g.excluded = excluded ? W.excluded.d : nullptr; g.C = C; g.k = k; g.min_gain = min_gain;
    g.L = W.L.d; g.order = W.order.d; g.gains = W.gains.d; g.pick_var = W.pick_var.d; g.remaining = W.remaining.d; g.picked = W.picked.d;
    hipLaunchKernelGGL(k_sel_greedy, dim3(1), dim3(kThreads), 0, st, g);
    HIP_CHECK(hipGetLastError());
    std::vector<double> part((size_t)pairs), gains((size_t)k);
    int32_t picked = 0;
    staged_d2h(part.data(), W.part.d, (size_t)pairs * sizeof(double), st);
    staged_d2h(gains.data(), W.gains.d, (size_t)k * sizeof(double), st);
    staged_d2h(&picked, W.picked.d, sizeof(int32_t), st);
    if (out.order) staged_d2h(out.order, W.order.d, (size_t)k * sizeof(int32_t), st);
    if (out.pick_variances) staged_d2h(out.pick_variances, W.pick_var.d, (size_t)k * sizeof(double), st);
    if (out.remaining) staged_d2h(out.remaining, W.remaining.d, (size_t)C * sizeof(double), st);
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

// What score_refine_select_ranges does with a solved block of lv_pair_solve, and with all of them.
struct SelCross {
    const double* precisions; int32_t k; double min_gain;
    SelOutputs out; double* matrix; score_select_info* info;
    SelWork* W = nullptr;
    SelCrossArgs a{};
    bool pending = false;
    double cross_ms = 0.0;
    void settle() {   // (the block's own read of its residuals has waited for the stream)
        if (!pending) return;
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, W->ev0, W->ev1));
        cross_ms += ms;
        pending = false;
    }
    void check(int32_t n_pairs, const std::string& who) { sel_check(n_pairs, k, min_gain, precisions, who); }
    template <class Refine>
    void begin(Refine& R, const LvPairArgs& l, int32_t n_pairs, hipStream_t st) {
        W = &R.sel;
        W->reserve(n_pairs, k);
        if (!W->ev0) { HIP_CHECK(hipEventCreate(&W->ev0)); HIP_CHECK(hipEventCreate(&W->ev1)); }
        staged_h2d(W->w.d, precisions, (size_t)n_pairs * sizeof(double), st);
        a.v = l.v; a.x = l.x; a.n = l.n; a.pa = l.pa; a.pb = l.pb; a.C = n_pairs; a.P = W->P.d;
    }
    template <class Refine>
    void block(Refine& R, int c0, int live, hipStream_t st) {
        settle();
        a.c0 = c0;
        HIP_CHECK(hipEventRecord(W->ev0, st));
        gn_dim(R.P.dim, [&](auto dim) {
            hipLaunchKernelGGL(k_sel_cross<decltype(dim)::value>, dim3((unsigned)((a.C + kThreads - 1) / kThreads), (unsigned)live),
                               dim3(kThreads), 0, st, a);
        });
        HIP_CHECK(hipEventRecord(W->ev1, st));
        pending = true;
    }
    // col_done: 1 where the column converged; the others' candidates are excluded
    void end(const std::vector<int32_t>& col_done, hipStream_t st) {
        settle();
        const int32_t C = a.C;
        const double t0 = now_ms();
        if (matrix) staged_d2h(matrix, W->P.d, (size_t)C * (size_t)C * sizeof(double), st);
        std::vector<int32_t> excluded((size_t)C);
        int32_t n_excluded = 0;
        for (int32_t c = 0; c < C; ++c) n_excluded += excluded[(size_t)c] = col_done[(size_t)c] ? 0 : 1;
        double asymmetry = 0.0, total = 0.0;
        const int32_t picked = sel_run(*W, C, k, min_gain, n_excluded ? excluded.data() : nullptr, out, &asymmetry, &total, st);
        if (info) {
            info->candidates = C; info->picked = picked; info->excluded = n_excluded; info->total_gain = total;
            info->asymmetry = asymmetry; info->cross_ms = cross_ms; info->greedy_ms = now_ms() - t0;
        }
    }
};

// score_select_greedy: the selection on a caller's matrix, buffers of its own
inline void sel_greedy_alone(const double* matrix, const double* precisions, const int32_t* excluded, int32_t n, int32_t k,
                             double min_gain, const SelOutputs& out, int32_t* picked, double* asymmetry) {
    const std::string who = "score_select_greedy: ";
    sel_check(n, k, min_gain, precisions, who);
    if (!matrix) throw std::runtime_error(who + "the matrix is missing");
    hipStream_t st = nullptr;
    SelWork W;
    W.reserve(n, k);
    staged_h2d(W.P.d, matrix, (size_t)n * (size_t)n * sizeof(double), st);
    staged_h2d(W.w.d, precisions, (size_t)n * sizeof(double), st);
    const int32_t got = sel_run(W, n, k, min_gain, excluded, out, asymmetry, nullptr, st);
    if (picked) *picked = got;
}

}  // namespace score

#endif  // __HIPCC__

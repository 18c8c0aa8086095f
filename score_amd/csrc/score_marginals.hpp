// score_marginals.hpp -- marginal covariances of the refined estimate (include/score_marginals.h): H X = E_S with
// H = J'J at the given point, one unit column per scalar unknown of the selected variables, by a chain-preconditioned
// conjugate-gradient iteration over BLOCKS of up to kMvMaxWidth columns that advance in lock-step.
//
// What exists already and is used as it is: the per-measurement blocks (k_gn_blocks<DIM>), the gather of H on the
// linear-mode handle's pattern (k_gn_gather_h, lambda = 0), the chain factorisation (derive_rho_data -> k_factor) and the
// application of M^-1 to several vectors in one launch (HipBackend::precondition_block: chains, the second level of
// score_join.hpp, Jacobi on the landmark columns; the loop-closure correction is left out -- the preconditioner only has to
// be one fixed SPD operator for the whole solve).  New here: the product over several vectors and the vector updates of the
// block.  Shared with the group's iteration (score_group_pcg.hpp) and the spectrum (score_spectrum.hpp): the tiles and the
// product of one tile (mv_tiles, MvTiles, mv_product_tile), the slot counts (mv_slots, mv_with_slots), the rule of the gated
// iteration (pcg_finite, pcg_step_rule, pcg_direction_rule: one rule, two engines -- the group needs k_gbm_rz so that no
// partial of r'z straddles members, this file takes r'z from the chain kernel's own partials), the variables' unknowns
// (mv_variable_unknowns) and the verdict of a call from its columns (mv_report).  Shared with the posterior samples
// (score_samples.hpp): the iteration itself (mv_block_pcg), from their own right-hand sides.  The refinement handle gives the
// head of a call (h_at_point) and the product's tiles (product_tiles: cut once, read here and by the spectrum).
//
// Vectors of a block are stored one after the other, stride n (the layout PrecArgs::vec_stride expects).  One iteration:
//   k_mv_product    w_c = H p_c for every live column from ONE pass over the CSR matrix, per-workgroup partials of p_c'w_c
//   k_mv_step       alpha_c = r'z / p'w (both re-reduced from the partials in a fixed order), x_c += alpha p_c, r_c -= alpha w_c
//   M^-1            z_c = M^-1 r_c and the chain kernel's own partials of r_c'z_c (precondition_block)
//   k_mv_direction  beta = r'z_new / r'z_old, p_c = z_c + beta p_c; the gate r'z_new <= rel_tol^2 r0'z0 raises the column's
//                   done word (the stopping rule of score_linear_solve)
// Every kernel tests the column's done word first and leaves a done column's x, r and p as they are (the chain kernel
// keeps writing the scratch z of such a column: it is never read again).  1: converged, 2: broken down (a non-finite r'z or
// p'w, or p'w <= 0) -- reported as not converged.  No atomics: every sum is a fixed-order reduction, and all workgroups of
// a column reduce the same partials in the same order, so they take the same decision.
//
// Rows are short (a pose row holds 3-6 unknowns and a dozen neighbours) except the landmark rows (a beacon ranged from
// every pose: 2 x poses entries).  A tile of the product is either kMvRows consecutive short rows, kMvLanes lanes each, or
// ONE long row spread over the workgroup and reduced through LDS.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/score_marginals.h"
#include "score_kernels.hpp"

namespace score {

constexpr int kMvMaxWidth = 16;                  // columns of a block
constexpr int kMvThreads = kThreads;
constexpr int kMvLanes = 4;                      // lanes of a short row
constexpr int kMvRows = kMvThreads / kMvLanes;   // short rows of a tile
constexpr int kMvLongRow = 128;                  // entries beyond which a row is a tile of its own
constexpr int kMvDone = 0, kMvIters = kMvMaxWidth, kMvZero = 2 * kMvMaxWidth, kMvFlagWords = 2 * kMvMaxWidth + 1;

struct MvArgs {
    // H on the linear-mode handle's pattern, and the product's tiles {first row, end row, long row?, 0}
    const int32_t* ptr; const int32_t* col; const double* val;
    const int4* tiles;
    int n_tiles;
    long long n;
    int32_t* flags;            // [kMvDone + c] done word, [kMvIters + c] steps executed, [kMvZero] a zero (the chain kernel's done word)
    int all_columns;           // product: ignore the done words (the residual's product H x)
    // vectors of the block, column c at c * n
    double* x; double* r; const double* z; double* p; double* w;
    const double* p_in;        // the product's operand (p, or x for the residual)
    double* pw_part;           // [c * n_tiles + tile]
    const double* rz_new;      // [c * n_prec + item]: partials of the last application of M^-1
    const double* rz_old;
    int n_prec;
    int first;                 // direction: p = z, the gate's threshold is set
    double tol2;
    double* ref;               // per column: rel_tol^2 r0'z0
    // right-hand sides, residuals, the rows of S
    const int32_t* sel;        // C selected unknowns
    int c0, live, C;           // the block's first column in sel, its live columns, all columns
    double* res_part;          // [c * gridDim.x + block]
    double* joint;             // C x C
};

// (the breakdown test of every gated iteration here and in score_group_pcg.hpp: neither infinite nor NaN)
__device__ __forceinline__ bool pcg_finite(double v) { return fabs(v) <= 1.79769313486231570e308; }

// The rule of the gated iteration, stated once: k_mv_step / k_mv_direction and k_gbm_step / k_gbm_direction
// (score_group_pcg.hpp) re-reduce their own partials into r'z and p'w, ask here, and write the verdict into their own words.
// The step: r'z and p'w finite and p'w > 0, then alpha = r'z / p'w; anything else is a breakdown (done word kPcgBroken).
__device__ __forceinline__ bool pcg_step_rule(double rz, double pw, double& alpha) {
    if (!(pcg_finite(rz) && pcg_finite(pw) && pw > 0.0)) return false;
    alpha = rz / pw;
    return true;
}
// The direction: kPcgGo -- p = z + beta p with beta = r'z_new / r'z_old; kPcgThreshold (the first direction) -- p = z and the
// gate's threshold becomes tol2 r'z_new; kPcgConverged and kPcgBroken are the done words.  ref: the slot's threshold word,
// read only where the gate is tested.
constexpr int kPcgGo = 0, kPcgConverged = 1, kPcgBroken = 2, kPcgThreshold = 3;
__device__ __forceinline__ int pcg_direction_rule(bool first, double rzn, double rzo, const double* ref, double& beta) {
    beta = 0.0;
    if (first) {  // (a zero right-hand side is solved by x = 0; anything else is no SPD preconditioner)
        if (!(pcg_finite(rzn) && rzn > 0.0)) return rzn == 0.0 ? kPcgConverged : kPcgBroken;
        return kPcgThreshold;
    }
    if (!(pcg_finite(rzn) && rzo > 0.0)) return kPcgBroken;
    if (rzn <= *ref) return kPcgConverged;
    beta = rzn / rzo;
    return kPcgGo;
}

// the slots a block of `most` live columns runs in, and f(std::integral_constant<int, NV>) for that count: the product kernels
// are compiled for 1, 2, 4, 8 and 16 vectors
inline int mv_slots(int most) { return most <= 1 ? 1 : most <= 2 ? 2 : most <= 4 ? 4 : most <= 8 ? 8 : 16; }
template <class F>
inline void mv_with_slots(int NV, F f) {
    switch (NV) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        default: f(std::integral_constant<int, 16>{}); break;
    }
}

// The product of one tile: w_c = H p_in_c for the columns of `live`, the tile's partial of p_in_c'w_c into
// pw_part[c * part_stride + part_slot].  Stated once: k_mv_product (the columns of one graph) and k_gbm_product
// (score_group_pcg.hpp: the slots of the tile's member inside a union) call it with their live mask and partial slot.
// NV: vectors of the block (compile time: the sums live in registers).  red: (kMvThreads / 64) * NV doubles of LDS.  Every
// lane of the workgroup enters with the same tile and the same (non-empty) mask.
template <int NV>
__device__ __forceinline__ void mv_product_tile(const int32_t* ptr, const int32_t* col, const double* val, const int4 tile, const long long n,
                                                const double* p_in, double* w, double* pw_part, const size_t part_stride,
                                                const size_t part_slot, const unsigned live, double* red) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double acc[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) acc[c] = 0.0;
    if (tile.z) {  // one long row over the workgroup
        const int row = tile.x;
        const int k1 = ptr[row + 1];
        for (int k = ptr[row] + t; k < k1; k += kMvThreads) {
            const double v = val[k];
            const long long j = col[k];
#pragma unroll
            for (int c = 0; c < NV; ++c)
                if (live >> c & 1) acc[c] += v * p_in[c * n + j];
        }
#pragma unroll
        for (int c = 0; c < NV; ++c)
            if (live >> c & 1) {
                const double s = wave_sum(acc[c]);
                if (lane == 0) red[wave * NV + c] = s;
            }
        __syncthreads();
        if (t < NV && (live >> t & 1)) {
            const double wv = (red[t] + red[NV + t]) + (red[2 * NV + t] + red[3 * NV + t]);
            w[t * n + row] = wv;
            pw_part[(size_t)t * part_stride + part_slot] = p_in[t * n + row] * wv;
        }
        return;
    }
    // short rows: kMvLanes lanes per row, their sums joined as (l0 + l1) + (l2 + l3)
    const int row = tile.x + t / kMvLanes, sub = t % kMvLanes;
    const bool mine = row < tile.y;
    if (mine) {
        const int k1 = ptr[row + 1];
        for (int k = ptr[row] + sub; k < k1; k += kMvLanes) {
            const double v = val[k];
            const long long j = col[k];
#pragma unroll
            for (int c = 0; c < NV; ++c)
                if (live >> c & 1) acc[c] += v * p_in[c * n + j];
        }
    }
#pragma unroll
    for (int c = 0; c < NV; ++c)
        if (live >> c & 1) {
            double s = acc[c];
            s += __shfl_xor(s, 1, 64);
            s += __shfl_xor(s, 2, 64);
            double pw = 0.0;
            if (mine && sub == 0) {
                w[c * n + row] = s;
                pw = p_in[c * n + row] * s;
            }
            pw = wave_sum(pw);
            if (lane == 0) red[wave * NV + c] = pw;
        }
    __syncthreads();
    if (t < NV && (live >> t & 1))
        pw_part[(size_t)t * part_stride + part_slot] = (red[t] + red[NV + t]) + (red[2 * NV + t] + red[3 * NV + t]);
}

// w_c = H p_in_c over the live columns, partials of p_in_c'w_c
template <int NV>
__global__ __launch_bounds__(kMvThreads) void k_mv_product(MvArgs a) {
    __shared__ double red[(kMvThreads / 64) * NV];
    unsigned live = 0;
#pragma unroll
    for (int c = 0; c < NV; ++c)
        if (a.all_columns || a.flags[kMvDone + c] == 0) live |= 1u << c;
    if (!live) return;
    mv_product_tile<NV>(a.ptr, a.col, a.val, a.tiles[blockIdx.x], a.n, a.p_in, a.w, a.pw_part, (size_t)a.n_tiles, (size_t)blockIdx.x, live, red);
}

// grid (row blocks, columns): alpha = r'z / p'w ; x += alpha p ; r -= alpha w
__global__ __launch_bounds__(kMvThreads) void k_mv_step(MvArgs a) {
    __shared__ double red[8];
    const int c = blockIdx.y, t = threadIdx.x;
    if (a.flags[kMvDone + c]) return;
    double rz = 0.0, pw = 0.0;
    for (int i = t; i < a.n_prec; i += kMvThreads) rz += a.rz_new[(size_t)c * a.n_prec + i];
    for (int i = t; i < a.n_tiles; i += kMvThreads) pw += a.pw_part[(size_t)c * a.n_tiles + i];
    block_sum2(rz, pw, red);
    const bool lead = blockIdx.x == 0 && t == 0;
    double alpha;
    if (!pcg_step_rule(rz, pw, alpha)) {
        if (lead) a.flags[kMvDone + c] = kPcgBroken;
        return;
    }
    const long long i = (long long)blockIdx.x * kMvThreads + t;
    if (i < a.n) {
        const long long e = c * a.n + i;
        a.x[e] += alpha * a.p[e];
        a.r[e] -= alpha * a.w[e];
    }
    if (lead) a.flags[kMvIters + c] += 1;
}

// grid (row blocks, columns): the gate, then p = z + beta p (first: p = z and the gate's threshold)
__global__ __launch_bounds__(kMvThreads) void k_mv_direction(MvArgs a) {
    __shared__ double red[8];
    const int c = blockIdx.y, t = threadIdx.x;
    if (a.flags[kMvDone + c]) return;
    double rzn = 0.0, rzo = 0.0;
    for (int i = t; i < a.n_prec; i += kMvThreads) {
        rzn += a.rz_new[(size_t)c * a.n_prec + i];
        if (!a.first) rzo += a.rz_old[(size_t)c * a.n_prec + i];
    }
    block_sum2(rzn, rzo, red);
    const bool lead = blockIdx.x == 0 && t == 0;
    double beta;
    const int verdict = pcg_direction_rule(a.first != 0, rzn, rzo, a.ref + c, beta);
    if (verdict == kPcgConverged || verdict == kPcgBroken) {
        if (lead) a.flags[kMvDone + c] = verdict;
        return;
    }
    if (verdict == kPcgThreshold && lead) a.ref[c] = a.tol2 * rzn;
    const long long i = (long long)blockIdx.x * kMvThreads + t;
    if (i < a.n) {
        const long long e = c * a.n + i;
        a.p[e] = a.first ? a.z[e] : a.z[e] + beta * a.p[e];
    }
}

// grid (row blocks, columns): x = 0, r = the unit vector of the column's unknown (columns beyond `live`: zero, done from the start)
__global__ __launch_bounds__(kMvThreads) void k_mv_rhs(MvArgs a) {
    const int c = blockIdx.y, t = threadIdx.x;
    const long long i = (long long)blockIdx.x * kMvThreads + t;
    const bool on = c < a.live;
    if (i < a.n) {
        a.x[c * a.n + i] = 0.0;
        a.r[c * a.n + i] = (on && i == a.sel[a.c0 + c]) ? 1.0 : 0.0;
    }
    if (blockIdx.x == 0 && t == 0) {
        a.flags[kMvDone + c] = on ? 0 : 1;
        a.flags[kMvIters + c] = 0;
        if (c == 0) a.flags[kMvZero] = 0;
    }
}

// grid (row blocks, live columns): partials of |e_c - w_c|^2 with w = H x
__global__ __launch_bounds__(kMvThreads) void k_mv_residual(MvArgs a) {
    __shared__ double red[4];
    const int c = blockIdx.y, t = threadIdx.x;
    const long long i = (long long)blockIdx.x * kMvThreads + t;
    double d = 0.0;
    if (i < a.n) d = (i == a.sel[a.c0 + c] ? 1.0 : 0.0) - a.w[c * a.n + i];
    const double s = block_sum(d * d, red);
    if (t == 0) a.res_part[(size_t)c * gridDim.x + blockIdx.x] = s;
}

// grid (blocks over the C rows of S, live columns): joint[s, c0 + c] = x_c[sel[s]]
__global__ __launch_bounds__(kMvThreads) void k_mv_gather(MvArgs a) {
    const int c = blockIdx.y;
    const long long s = (long long)blockIdx.x * kMvThreads + threadIdx.x;
    if (s < a.C) a.joint[s * a.C + a.c0 + c] = a.x[c * a.n + a.sel[s]];
}

// the product's tiles {first row, end row, long row?, member} from the row pointers of a graph's n rows, appended; row0:
// where the graph's rows start (a member of a union, score_gn_batch.hpp: its first unknown)
inline void mv_tiles(const std::vector<int32_t>& ptr, int64_t n, std::vector<int4>& tiles, int64_t row0 = 0, int member = 0) {
    auto len = [&](int64_t i) { return ptr[(size_t)i + 1] - ptr[(size_t)i]; };
    int64_t row = 0;
    while (row < n) {
        if (len(row) > kMvLongRow) { tiles.push_back(make_int4((int)(row0 + row), (int)(row0 + row + 1), 1, member)); ++row; continue; }
        int64_t end = row;
        while (end < n && end - row < kMvRows && len(end) <= kMvLongRow) ++end;
        tiles.push_back(make_int4((int)(row0 + row), (int)(row0 + end), 0, member));
        row = end;
    }
}

// Tiles on the device: cut by mv_tiles from a graph's row pointers (add: once per member of a union, appended), sent once.
struct MvTiles {
    DevBuf<int4> dev;
    int n = 0;
    std::vector<int4> cut;  // on the host until they are sent
    void add(const std::vector<int32_t>& ptr, int64_t rows, int64_t row0 = 0, int member = 0) { mv_tiles(ptr, rows, cut, row0, member); }
    void send(hipStream_t st) {
        n = (int)cut.size();
        dev.alloc(cut.size());
        staged_h2d(dev.d, cut.data(), cut.size() * sizeof(int4), st);
        std::vector<int4>().swap(cut);
    }
};

// The verdict of a call from its columns (or draws), stated once for mv_solve, ps_solve, gbm_solve and gbs_solve: a column
// that is not done counts as unconverged; worst is the largest residual, infinite where one is not finite; the caller's
// iters get the steps of a done column and -(steps + 1) of any other.  Returns the unconverged columns.
inline int mv_report(const std::vector<int32_t>& done, const std::vector<int32_t>& steps, const std::vector<double>& res, double* residuals,
                     int32_t* iters, double& worst) {
    int unconverged = 0;
    worst = 0.0;
    for (size_t c = 0; c < done.size(); ++c) {
        if (!done[c]) ++unconverged;
        worst = std::isfinite(res[c]) ? std::max(worst, res[c]) : INFINITY;
        if (residuals) residuals[c] = res[c];
        if (iters) iters[c] = done[c] ? steps[c] : -(steps[c] + 1);
    }
    return unconverged;
}

// The unknowns of the selected variables of one graph -- Np poses of dp unknowns each (pose 0 is fixed), then Nl landmarks of
// dim -- appended to sel in the order of include/score_marginals.h.  who: the entry point's words in front of a message.
inline void mv_variable_unknowns(int64_t Np, int64_t Nl, int dp, int dim, const int32_t* vars, int32_t n_vars, const std::string& who,
                                 std::vector<int32_t>& sel) {
    std::vector<char> seen((size_t)(Np + Nl), 0);
    for (int32_t k = 0; k < n_vars; ++k) {
        const int64_t v = vars[k];
        if (v < 0 || v >= Np + Nl) throw std::runtime_error(who + "variable out of range");
        if (v == 0) throw std::runtime_error(who + "pose 0 is fixed, it has no covariance");
        if (seen[(size_t)v]) throw std::runtime_error(who + "a variable is listed twice");
        seen[(size_t)v] = 1;
        const int64_t first = v < Np ? (int64_t)dp * (v - 1) : (int64_t)dp * (Np - 1) + (int64_t)dim * (v - Np);
        const int cnt = v < Np ? dp : dim;
        for (int a = 0; a < cnt; ++a) sel.push_back((int32_t)(first + a));
    }
}

inline void mv_columns(const GnProblem& P, const int32_t* vars, int32_t n_vars, std::vector<int32_t>& sel) {
    if (!vars || n_vars <= 0) throw std::runtime_error("score_refine_marginals: no variables");
    sel.clear();
    mv_variable_unknowns(P.Np, P.Nl, P.dp(), P.dim, vars, n_vars, "score_refine_marginals: ", sel);
}

// The block's buffers: they stay with the refinement handle between calls (device allocations of their own, not the
// handle's arena: they come with the first call and go with the handle).
struct MvWork {
    DevBuf<double> x, r, z, p, w, p_scratch, pw_part, rz0, rz1, ref, res_part, zb;
    DevBuf<int32_t> flags;
    const int4* tiles = nullptr;  // the product's tiles: the handle's (T), shared with the spectrum
    int n_tiles = 0;
    void reserve(const GnProblem& P, const MvTiles& T, int n_prec, int zb_per_vector, hipStream_t st) {
        if (x.d) return;
        NoArena no_arena;
        tiles = T.dev.d; n_tiles = T.n;
        const size_t nv = (size_t)kMvMaxWidth, n = (size_t)P.n, rb = (n + kMvThreads - 1) / kMvThreads;
        DevBuf<double>* vecs[] = {&x, &r, &z, &p, &w, &p_scratch};
        for (DevBuf<double>* v : vecs) { v->alloc(nv * n); v->zero(st); }
        pw_part.alloc(nv * (size_t)n_tiles); pw_part.zero(st);
        // (every workgroup of a chain-kernel launch has a slot, per vector)
        rz0.alloc(nv * (size_t)n_prec + 4096); rz0.zero(st);
        rz1.alloc(nv * (size_t)n_prec + 4096); rz1.zero(st);
        ref.alloc(nv); ref.zero(st);
        res_part.alloc(nv * rb); res_part.zero(st);
        zb.alloc(nv * (size_t)std::max(1, zb_per_vector)); zb.zero(st);
        flags.alloc((size_t)kMvFlagWords); flags.zero(st);
    }
};

// w_c = H p_in_c as `m` says, compiled for NV vectors
inline void mv_launch_product(const MvArgs& m, int NV, hipStream_t st) {
    mv_with_slots(NV, [&](auto nv) {
        hipLaunchKernelGGL(k_mv_product<decltype(nv)::value>, dim3((unsigned)m.n_tiles), dim3(kMvThreads), 0, st, m);
    });
}

// The gated iteration of a block whose x, r and done words are set (k_mv_rhs here, k_ps_begin of score_samples.hpp): the
// first application of M^-1 and direction, then at most max_iters iterations queued in chunks.  flags: the block's words as
// last read.  Stated once: the marginals' columns and the posterior samples' draws both run it.
inline void mv_block_pcg(HipBackend& be, MvWork& W, MvArgs& a, int NV, int n_rblocks, int max_iters, std::vector<int32_t>& flags,
                         hipStream_t st) {
    // z = M^-1 r of every column of the block, the chain kernel's partials of r'z into `rz`
    auto precondition = [&](double* rz) {
        be.precondition_block(W.r.d, W.z.d, W.p_scratch.d, W.w.d, NV, a.n, W.flags.d + kMvZero, rz, W.zb.d);
    };
    double* rz_cur = W.rz0.d; double* rz_nxt = W.rz1.d;
    precondition(rz_cur);
    a.first = 1; a.rz_new = rz_cur; a.rz_old = nullptr;
    hipLaunchKernelGGL(k_mv_direction, dim3((unsigned)n_rblocks, (unsigned)NV), dim3(kMvThreads), 0, st, a);
    a.first = 0;
    queue_in_chunks(max_iters, [&]() {
        a.all_columns = 0; a.p_in = W.p.d;
        mv_launch_product(a, NV, st);
        a.rz_new = rz_cur;
        hipLaunchKernelGGL(k_mv_step, dim3((unsigned)n_rblocks, (unsigned)NV), dim3(kMvThreads), 0, st, a);
        precondition(rz_nxt);
        a.rz_new = rz_nxt; a.rz_old = rz_cur;
        hipLaunchKernelGGL(k_mv_direction, dim3((unsigned)n_rblocks, (unsigned)NV), dim3(kMvThreads), 0, st, a);
        std::swap(rz_cur, rz_nxt);
    }, [&]() {
        staged_d2h(flags.data(), W.flags.d, (size_t)kMvFlagWords * sizeof(int32_t), st);
        return std::all_of(flags.begin() + kMvDone, flags.begin() + kMvDone + NV, [](int32_t f) { return f != 0; });
    });
}

// The block's MvArgs on a refinement handle's matrix and buffers (the caller adds its own right-hand sides and outputs)
inline MvArgs mv_block_args(HipBackend& be, MvWork& W, long long n, double rel_tol) {
    MvArgs a{};
    a.ptr = be.Kset.mat.ptr.d; a.col = be.Kset.mat.col.d; a.val = be.Kset.mat.val.d;
    a.tiles = W.tiles; a.n_tiles = W.n_tiles; a.n = n; a.flags = W.flags.d;
    a.x = W.x.d; a.r = W.r.d; a.z = W.z.d; a.p = W.p.d; a.w = W.w.d; a.pw_part = W.pw_part.d;
    a.n_prec = be.n_prec; a.tol2 = rel_tol * rel_tol; a.ref = W.ref.d; a.res_part = W.res_part.d;
    return a;
}

// The solve.  Refine: score_refine (its point, blocks and gather, its linear-mode handle, its MvWork).
template <class Refine>
int mv_solve(Refine& R, const double* poses, const double* landmarks, const int32_t* vars, int32_t n_vars, double rel_tol,
             int32_t max_iters, int32_t block_width, double* joint, double* residuals, int32_t* iters, score_marginals_info* info) {
    const GnProblem& P = R.P;
    if (block_width < 0 || block_width > kMvMaxWidth) throw std::runtime_error("score_refine_marginals: block_width must be 0..16");
    if (!(rel_tol > 0.0) || max_iters < 1) throw std::runtime_error("score_refine_marginals: rel_tol must be positive and max_iters >= 1");
    std::vector<int32_t> sel;
    mv_columns(P, vars, n_vars, sel);
    const int C = (int)sel.size();
    if ((size_t)C * (size_t)C > ((size_t)1 << 27)) throw std::runtime_error("score_refine_marginals: too many columns for one call (C x C doubles beyond 1 GiB)");
    HipBackend& be = R.be();
    hipStream_t st = R.stream();
    const long long n = P.n;
    const double t0 = now_ms();
    // H at the point, on the handle's pattern; the chains factored once for the block path (the single solves factor per call)
    const bool seq = block_width == 0;
    R.h_at_point(poses, landmarks, "score_refine_marginals: ", seq ? nullptr : "blocks of columns need");
    if (!seq) be.derive_rho_data(false);
    const int NV = seq ? 1 : mv_slots(block_width);
    auto& W = R.mv;
    W.reserve(P, R.product_tiles(), be.n_prec, be.H->bs * be.n_join_seps, st);
    DevBuf<int32_t> d_sel;
    DevBuf<double> d_joint;
    {
        NoArena no_arena;
        d_sel.alloc((size_t)C); d_joint.alloc((size_t)C * (size_t)C);
    }
    staged_h2d(d_sel.d, sel.data(), (size_t)C * sizeof(int32_t), st);
    const int n_rblocks = (int)((n + kMvThreads - 1) / kMvThreads);
    MvArgs a = mv_block_args(be, W, n, rel_tol);
    a.sel = d_sel.d; a.C = C; a.joint = d_joint.d;
    const double t1 = now_ms();
    std::vector<int32_t> flags((size_t)kMvFlagWords), col_done((size_t)C, 0), col_iters((size_t)C, 0);
    std::vector<double> res_part((size_t)NV * (size_t)n_rblocks), col_res((size_t)C, 0.0);
    int batches = 0, pcg_iters = 0;
    const int width = seq ? 1 : block_width;
    for (int c0 = 0; c0 < C; c0 += width) {
        const int live = std::min(width, C - c0);
        a.c0 = c0; a.live = live;
        hipLaunchKernelGGL(k_mv_rhs, dim3((unsigned)n_rblocks, (unsigned)NV), dim3(kMvThreads), 0, st, a);
        if (seq) {
            // the single-right-hand-side solve of linear mode, as it is; its solution into the block's column 0
            int used = 0;
            const bool ok = be.linear_solve_core(R.lin->solver.H, W.r.d, rel_tol, max_iters, &used);
            HIP_CHECK(hipMemcpyAsync(W.x.d, be.xtu.d, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
            flags[kMvDone] = ok ? 1 : 0; flags[kMvIters] = used;
        } else {
            mv_block_pcg(be, W, a, NV, n_rblocks, max_iters, flags, st);
        }
        // the true residual of every column of the block (one more product, w = H x), the rows of S
        a.all_columns = 1; a.p_in = W.x.d;
        mv_launch_product(a, NV, st);
        hipLaunchKernelGGL(k_mv_residual, dim3((unsigned)n_rblocks, (unsigned)live), dim3(kMvThreads), 0, st, a);
        hipLaunchKernelGGL(k_mv_gather, dim3((unsigned)((C + kMvThreads - 1) / kMvThreads), (unsigned)live), dim3(kMvThreads), 0, st, a);
        HIP_CHECK(hipGetLastError());
        staged_d2h(res_part.data(), W.res_part.d, (size_t)live * (size_t)n_rblocks * sizeof(double), st);
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
    if (joint) staged_d2h(joint, d_joint.d, (size_t)C * (size_t)C * sizeof(double), st);
    HIP_CHECK(sync_stream(st));
    const double t2 = now_ms();
    double worst = 0.0;
    const int unconverged = mv_report(col_done, col_iters, col_res, residuals, iters, worst);
    if (info) {
        info->columns = C; info->batches = batches; info->pcg_iters = pcg_iters; info->unconverged = unconverged;
        info->max_residual = worst; info->setup_ms = t1 - t0; info->solve_ms = t2 - t1;
    }
    return unconverged ? 1 : 0;
}

}  // namespace score

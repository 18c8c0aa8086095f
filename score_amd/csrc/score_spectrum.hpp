// score_spectrum.hpp -- the lowest eigenpairs of the information matrix H = J'J at a point of a refinement handle
// (include/score_spectrum.h): LOBPCG (Knyazev 2001) with a block of kSpBlock = 16 vectors on A = H + sigma I.
//
// What exists already and is used as it is: the per-measurement blocks and the gather of H on the linear-mode handle's
// pattern (gather_h(sigma)), the chain factorisation (derive_rho_data), the application of M^-1 to 16 vectors in one launch
// (HipBackend::precondition_block, which mv_solve of score_marginals.hpp calls too: depth join, no loop-closure
// correction) and the product over 16 vectors (k_mv_product<16>, all_columns = 1).  M is the chain
// part of A -- tridiagonal pose blocks per chain, diagonal blocks of the landmarks -- and exists for a singular H because of
// the shift.  New here: the Gram kernel, the combine kernel, and the small kernels around them (start block, residuals,
// done words, max diag H).  Stated here once for a graph and for the members of a group (score_spectrum_batch.hpp): the
// start block's hash (sp_start_value), the directions in use (sp_active_mask), one row tile of the Gram pass and the store
// of its partial matrices (sp_gram_tile, sp_gram_store).  The handle's head of a call and its product tiles: h_at_point,
// product_tiles (score_marginals.hpp).
//
// The six blocks X, W, P (S) and AX, AW, AP (AS) are n x 16 each, column c at c * n (the layout PrecArgs::vec_stride
// expects).  One iteration:
//   k_sp_residual   R_c = AX_c - theta_c X_c, per-workgroup partials of |R_c|^2
//   k_sp_done       |R_c| re-reduced in a fixed order; done word of column c: |R_c| <= rel_tol * h_max (recomputed every
//                   iteration: soft locking -- a done column stays in X and in the Rayleigh-Ritz basis, its W and P leave)
//   launch_prec     W = M^-1 R, all 16 columns in one launch
//   k_mv_product    AW = A W.  AX and AP are NOT products: they follow X and P through the combine step (the same linear
//                   combination of AS that forms X and P from S), which saves two of three passes over the matrix; the
//                   drift this recurrence accumulates is bounded by a true product A X whenever the first k columns
//                   look done -- the iteration ends only on residuals of that product, and goes on with it otherwise
//   k_sp_gram       S'AS and S'S (48 x 48 each) from ONE pass over the six blocks, per-workgroup partials;
//   k_sp_gram_sum   the partials re-reduced in workgroup order.  No atomics anywhere: two calls give the same bits
//   (host)          both matrices and the 16 norms in one read (37 KB); Rayleigh-Ritz in score_spectrum_rr.hpp
//   k_sp_combine    X <- S C, P <- [W | P] C_wp (grid.y = 0) and AX <- (AS) C, AP <- [AW | AP] C_wp (grid.y = 1): six blocks
//                   read, four written, C (48 x 16) broadcast from LDS
// Every kernel of the iteration tests the done words first: a done column's W / P (and AW / AP) is neither read by the Gram
// and combine kernels -- it enters both as zero -- nor needed (the chain kernel keeps writing it, as in score_marginals.hpp).
//
// The Gram kernel: plain FMAs over an LDS-staged row tile, not v_mfma_f64_16x16x4_f64.  The pass moves 96 doubles per row
// and does 2 x 48 x 48 FMAs on them; at the headline n = 60 000 that is 46 MB and 0.28 GFMA -- the kernel is bound by the
// read of the six blocks and by launch latency, not by arithmetic (the vector units do the FMAs in a few microseconds), so
// the matrix cores would buy nothing, and the FMA form has a summation order that is plain to read: rows in order inside a
// workgroup, workgroups in order in k_sp_gram_sum.  A tile is kSpRows = 32 rows of all 96 columns, staged column-major with a
// leading dimension of 33 doubles: lanes load 32 consecutive rows of one column (256 contiguous bytes; a column starts at
// c * n, which is 16-byte aligned only for even n, so the loads stay 8 bytes wide), and in the FMA loop the 16 lanes that
// differ in their column triple are 3 * 33 = 99 doubles apart -- 198 banks, 6 modulo 64: sixteen distinct even banks, no
// conflict; the other lanes of the wavefront read the same addresses (broadcast).  Thread (ti, tj) of the 16 x 16 workgroup
// owns the 3 x 3 entries (3 ti + a, 3 tj + b) of both matrices: 18 accumulators, 9 LDS reads per row.  25 KB of LDS per
// workgroup leaves six workgroups per CU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/score_spectrum.h"
#include "score_marginals.hpp"
#include "score_spectrum_rr.hpp"

namespace score {

constexpr int kSpBlock = 16;                 // vectors iterated
constexpr int kSpM = 3 * kSpBlock;           // columns of S = [X | W | P]
constexpr int kSpRows = 32;                  // rows of a Gram tile
constexpr int kSpLd = kSpRows + 1;           // its leading dimension in LDS
constexpr int kSpGramWgs = 128;              // workgroups of the Gram pass at most (= partial matrices)
constexpr int kSpGramOut = 2 * kSpM * kSpM;  // S'AS then S'S
constexpr int kSpMinN = kSpM;                // below this S cannot have full rank

struct SpTheta { double v[kSpBlock]; };

struct SpArgs {
    long long n;
    double* S[3];            // X, W, P
    double* AS[3];           // AX, AW, AP
    double* R;               // residual block, the preconditioner's operand
    int32_t* flags;          // [c] done word of column c, [kSpBlock] a zero (the chain kernel's done word)
    int x_only;              // Gram / combine: W and P are not in use (orthonormalisation of the start block)
    int has_p;               // P holds directions
    double tol;              // rel_tol * h_max
    double* res_part;        // [c * n_rblocks + block]
    int n_rblocks;
    double* gram_part;       // [workgroup][2][48][48]
    int n_gram_wgs, n_row_tiles;
    double* out;             // [2][48][48] S'AS, S'S; then the 16 residual norms
    const double* coef;      // 48 x 16 row-major
};

// The bodies below are stated once for a graph and for a group: the kernels here and their k_gsp_ twins
// (score_spectrum_batch.hpp) call them with their own row range, flags and coefficients.

// the directions of S in use, bit b * 16 + c for block b, column c; flags: the 16 done words of the graph (of the member)
__device__ __forceinline__ unsigned long long sp_active_mask(int x_only, int has_p, const int32_t* flags) {
    unsigned long long act = 0xFFFFull;
    if (x_only) return act;
#pragma unroll
    for (int c = 0; c < kSpBlock; ++c)
        if (flags[c] == 0) act |= (1ull << (kSpBlock + c)) | (has_p ? 1ull << (2 * kSpBlock + c) : 0ull);
    return act;
}

// entry (i, c) of the start block: a fixed integer hash of (unknown, column), in (-1, 1); i is member-local in a group
__device__ __forceinline__ double sp_start_value(long long i, int c) {
    unsigned long long h = (unsigned long long)i * kSpBlock + (unsigned long long)c + 0x9E3779B97F4A7C15ull;
    h = (h ^ (h >> 30)) * 0xBF58476D1CE4E5B9ull;
    h = (h ^ (h >> 27)) * 0x94D049BB133111EBull;
    h ^= h >> 31;
    return (double)(h >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

// One row tile of the Gram pass (the head of the file): rows row0 .. row0 + 31 of the n_rows rows that start at `base` in
// every column (column c of a block at c * stride) are staged into s and as -- a row beyond n_rows or a direction out of
// use as zero --, then thread (ti, tj) adds the tile's rows IN ROW ORDER to its 3 x 3 entries (3 ti + x, 3 tj + y) of S'AS
// (ga) and S'S (gb).  Every lane of the workgroup enters; s and as may be staged again on return.
__device__ __forceinline__ void sp_gram_tile(double* const* S, double* const* AS, long long stride, long long base, long long row0,
                                             long long n_rows, unsigned long long act, double* s, double* as, double (&ga)[3][3],
                                             double (&gb)[3][3]) {
    const int t = threadIdx.x, tj = t & 15, ti = t >> 4;
    for (int e = t; e < 2 * kSpM * kSpRows; e += kMvThreads) {
        const int col = e / kSpRows, rr = e % kSpRows, cc = col % kSpM;
        const long long row = row0 + rr;
        double v = 0.0;
        if (row < n_rows && (act >> cc & 1)) {
            const double* src = col < kSpM ? S[cc / kSpBlock] : AS[cc / kSpBlock];
            v = src[(cc % kSpBlock) * stride + base + row];
        }
        (col < kSpM ? s : as)[cc * kSpLd + rr] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int rr = 0; rr < kSpRows; ++rr) {
        double si[3], sj[3], aj[3];
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            si[x] = s[(3 * ti + x) * kSpLd + rr];
            sj[x] = s[(3 * tj + x) * kSpLd + rr];
            aj[x] = as[(3 * tj + x) * kSpLd + rr];
        }
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y) {
                gb[x][y] += si[x] * sj[y];
                ga[x][y] += si[x] * aj[y];
            }
    }
    __syncthreads();
}

// the workgroup's partial matrices, S'AS then S'S, 48 x 48 row-major each
__device__ __forceinline__ void sp_gram_store(double* part, const double (&ga)[3][3], const double (&gb)[3][3]) {
    const int t = threadIdx.x, tj = t & 15, ti = t >> 4;
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y) {
            const int e = (3 * ti + x) * kSpM + 3 * tj + y;
            part[e] = ga[x][y];
            part[kSpM * kSpM + e] = gb[x][y];
        }
}

// grid (row blocks, 16): the start block (sp_start_value of (unknown, column)); the done words cleared
__global__ __launch_bounds__(kMvThreads) void k_sp_start(SpArgs a) {
    const int c = blockIdx.y;
    const long long i = (long long)blockIdx.x * kMvThreads + threadIdx.x;
    if (i < a.n) a.S[0][c * a.n + i] = sp_start_value(i, c);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.flags[c] = 0;
        if (c == 0) a.flags[kSpBlock] = 0;
    }
}

// per-workgroup maxima of the diagonal of the gathered matrix
__global__ __launch_bounds__(kThreads) void k_sp_hmax(const double* __restrict__ val, const int32_t* __restrict__ is_diag, int64_t nnz,
                                                      double* __restrict__ part) {
    __shared__ double red[4];
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    double v = 0.0;
    if (k < nnz && is_diag[k]) v = val[k] == val[k] ? val[k] : INFINITY;  // (fmax would drop a NaN)
    v = block_max(v, red);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// grid (row blocks, 16): R_c = AX_c - theta_c X_c, partials of |R_c|^2
__global__ __launch_bounds__(kMvThreads) void k_sp_residual(SpArgs a, SpTheta th) {
    __shared__ double red[4];
    const int c = blockIdx.y;
    const long long i = (long long)blockIdx.x * kMvThreads + threadIdx.x;
    double d = 0.0;
    if (i < a.n) {
        const long long e = c * a.n + i;
        d = a.AS[0][e] - th.v[c] * a.S[0][e];
        a.R[e] = d;
    }
    const double s = block_sum(d * d, red);
    if (threadIdx.x == 0) a.res_part[(size_t)c * (size_t)a.n_rblocks + blockIdx.x] = s;
}

// one workgroup: the norms in a fixed order, the done words
__global__ __launch_bounds__(kThreads) void k_sp_done(SpArgs a) {
    __shared__ double red[4];
    for (int c = 0; c < kSpBlock; ++c) {
        const double s = reduce_partials(a.res_part + (size_t)c * (size_t)a.n_rblocks, 0, a.n_rblocks, red);
        if (threadIdx.x == 0) {
            const double nrm = sqrt(s);
            a.out[kSpGramOut + c] = nrm;
            a.flags[c] = nrm <= a.tol ? 1 : 0;  // (a non-finite norm is not done)
        }
    }
}

// S'AS and S'S of the directions in use, per-workgroup partials (see the head of the file)
__global__ __launch_bounds__(kMvThreads) void k_sp_gram(SpArgs a) {
    __shared__ double s[kSpM * kSpLd], as[kSpM * kSpLd];
    const unsigned long long act = sp_active_mask(a.x_only, a.has_p, a.flags);
    double ga[3][3] = {}, gb[3][3] = {};
    for (int tile = blockIdx.x; tile < a.n_row_tiles; tile += gridDim.x)  // (grid-stride: tiles in ascending order per workgroup)
        sp_gram_tile(a.S, a.AS, a.n, 0, (long long)tile * kSpRows, a.n, act, s, as, ga, gb);
    sp_gram_store(a.gram_part + (size_t)blockIdx.x * (size_t)kSpGramOut, ga, gb);
}

// grid (kSpGramOut / 256): the partial matrices summed in workgroup order
__global__ __launch_bounds__(kMvThreads) void k_sp_gram_sum(SpArgs a) {
    const int e = blockIdx.x * kMvThreads + threadIdx.x;
    if (e >= kSpGramOut) return;
    double acc = 0.0;
    for (int w = 0; w < a.n_gram_wgs; ++w) acc += a.gram_part[(size_t)w * (size_t)kSpGramOut + (size_t)e];
    a.out[e] = acc;
}

// grid (row blocks, 2), one row per lane: y = 0: X <- S C, P <- [W | P] C_wp; y = 1: the same combination of AS into AX, AP.
// A lane reads its row of all three blocks before it writes: in place.  (k_gsp_combine repeats the row's text: called through
// a function of its own the 32 sums take 98 VGPRs here, not 96, and one wave per SIMD less -- profiles/block_bodies_resources.md.)
__global__ __launch_bounds__(kMvThreads) void k_sp_combine(SpArgs a) {
    __shared__ double c[kSpM * kSpBlock];
    for (int e = threadIdx.x; e < kSpM * kSpBlock; e += kMvThreads) c[e] = a.coef[e];
    __syncthreads();
    const unsigned long long act = sp_active_mask(a.x_only, a.has_p, a.flags);
    const long long i = (long long)blockIdx.x * kMvThreads + threadIdx.x;
    if (i >= a.n) return;
    double* const* blk = blockIdx.y ? a.AS : a.S;
    double x[kSpBlock], p[kSpBlock];
#pragma unroll
    for (int j = 0; j < kSpBlock; ++j) x[j] = p[j] = 0.0;
    // (four loads in flight per lane; unrolled further the 32 sums no longer fit the registers of a 256-lane workgroup)
#pragma unroll 4
    for (int cc = 0; cc < kSpBlock; ++cc) {
        const double v = blk[0][cc * a.n + i];
#pragma unroll
        for (int j = 0; j < kSpBlock; ++j) x[j] += v * c[cc * kSpBlock + j];
    }
#pragma unroll 1
    for (int b = 1; b < 3; ++b)
#pragma unroll 4
        for (int cc = 0; cc < kSpBlock; ++cc) {
            if (!(act >> (b * kSpBlock + cc) & 1)) continue;
            const double v = blk[b][cc * a.n + i];
#pragma unroll
            for (int j = 0; j < kSpBlock; ++j) p[j] += v * c[(b * kSpBlock + cc) * kSpBlock + j];
        }
#pragma unroll
    for (int j = 0; j < kSpBlock; ++j) {
        blk[0][j * a.n + i] = x[j] + p[j];
        blk[2][j * a.n + i] = p[j];
    }
}

// The solver's buffers: they stay with the refinement handle between calls (device allocations of their own, as MvWork's).
struct SpWork {
    DevBuf<double> x, w, p, ax, aw, ap, r, p_scratch, pw_part, rz, zb, res_part, gram_part, out, coef, hmax_part;
    DevBuf<int32_t> flags;
    const int4* tiles = nullptr;  // the product's tiles: the handle's (T), shared with the marginals
    int n_tiles = 0, n_rblocks = 0, n_row_tiles = 0, n_gram_wgs = 0, n_hblocks = 0;
    void reserve(const GnProblem& P, const MvTiles& T, int n_prec, int zb_per_vector, int hblocks, hipStream_t st) {
        if (x.d) return;
        NoArena no_arena;
        tiles = T.dev.d; n_tiles = T.n;
        const size_t nv = (size_t)kSpBlock, n = (size_t)P.n;
        n_rblocks = (int)((n + kMvThreads - 1) / kMvThreads);
        n_row_tiles = (int)((n + kSpRows - 1) / kSpRows);
        n_gram_wgs = std::min(n_row_tiles, kSpGramWgs);
        n_hblocks = hblocks;
        DevBuf<double>* vecs[] = {&x, &w, &p, &ax, &aw, &ap, &r, &p_scratch};
        for (DevBuf<double>* v : vecs) { v->alloc(nv * n); v->zero(st); }
        pw_part.alloc(nv * (size_t)n_tiles); pw_part.zero(st);
        rz.alloc(nv * (size_t)n_prec + 4096); rz.zero(st);  // (every workgroup of a chain-kernel launch has a slot, per vector)
        zb.alloc(nv * (size_t)std::max(1, zb_per_vector)); zb.zero(st);
        res_part.alloc(nv * (size_t)n_rblocks); res_part.zero(st);
        gram_part.alloc((size_t)n_gram_wgs * (size_t)kSpGramOut); gram_part.zero(st);
        out.alloc((size_t)kSpGramOut + nv); out.zero(st);
        coef.alloc((size_t)kSpM * nv); coef.zero(st);
        hmax_part.alloc((size_t)std::max(1, hblocks)); hmax_part.zero(st);
        flags.alloc(nv + 1); flags.zero(st);
    }
};

// What a call of the iteration is about: whose words open its messages, the values the product reads, whether A may be
// indefinite (the Ritz step's test of the lowest value), and what follows the iteration while X and the product still stand.
// SpInformation: score_refine_spectrum, A = J'J + sigma I in the handle's own values.  score_curvature.hpp has the other.
struct SpInformation {
    static constexpr bool indefinite = false;
    const char* who = "score_refine_spectrum: ";
    template <class Refine>
    const double* product_values(Refine& R, double) { return R.be().Kset.mat.val.d; }  // (after gather_h(sigma) and the factors)
    template <class Refine, class Product>
    void after_iteration(Refine&, Product&, double) {}
};

// what the iteration reports beside its outputs: the fields score_spectrum_info and score_curvature_info share
struct SpOutcome {
    int iterations = 0, unconverged = 0;
    int column[kSpBlock] = {};  // pair j of the outputs is this column of X
    double h_max = 0.0, sigma = 0.0, worst = 0.0, setup_ms = 0.0, solve_ms = 0.0;
};

// The solve, one body for both operators.  Refine: score_refine (its point, blocks and gather, its linear-mode handle, its
// SpWork `sp`).  The preconditioner is that of J'J + sigma I whatever the product reads.
template <class Refine, class Op>
int sp_iterate(Refine& R, Op& op, const double* poses, const double* landmarks, int32_t k, double rel_tol, int32_t max_iters,
               double shift_rel, double* values, double* vectors, double* residuals, SpOutcome& outcome) {
    const GnProblem& P = R.P;
    const std::string who = op.who;
    if (k < 1 || k > kSpBlock) throw std::runtime_error(who + "k must be 1..16");
    if (!(rel_tol > 0.0) || !std::isfinite(rel_tol) || max_iters < 1)
        throw std::runtime_error(who + "rel_tol must be positive and max_iters >= 1");
    if (!(shift_rel > 0.0) || !std::isfinite(shift_rel)) throw std::runtime_error(who + "shift_rel must be positive");
    HipBackend& be = R.be();
    hipStream_t st = R.stream();
    const long long n = P.n;
    const double t0 = now_ms();
    // the point, the blocks, H and max diag H; then A = H + sigma I on the handle's pattern and its chain factors
    R.h_at_point(poses, landmarks, who, "the block needs");
    if (n < kSpMinN)
        throw std::runtime_error(who + "fewer than 48 unknowns -- use the dense solver (engine=\"python\") for a graph this small");
    auto& W = R.sp;
    W.reserve(P, R.product_tiles(), be.n_prec, be.H->bs * be.n_join_seps, R.n_hblocks, st);
    hipLaunchKernelGGL(k_sp_hmax, dim3((unsigned)W.n_hblocks), dim3(kThreads), 0, st, (const double*)be.K0d.d, (const int32_t*)R.is_diag.d,
                       (int64_t)P.hcol.size(), W.hmax_part.d);
    HIP_CHECK(hipGetLastError());
    std::vector<double> hpart((size_t)W.n_hblocks);
    staged_d2h(hpart.data(), W.hmax_part.d, hpart.size() * sizeof(double), st);
    double h_max = 0.0;
    for (double v : hpart) h_max = std::max(h_max, v);
    if (!(h_max > 0.0) || !std::isfinite(h_max)) throw std::runtime_error(who + "the diagonal of H is zero or not finite at this point");
    const double sigma = shift_rel * h_max, tol = rel_tol * h_max;
    R.gather_h(sigma);
    be.derive_rho_data(false);

    SpArgs a{};
    a.n = n;
    a.S[0] = W.x.d; a.S[1] = W.w.d; a.S[2] = W.p.d;
    a.AS[0] = W.ax.d; a.AS[1] = W.aw.d; a.AS[2] = W.ap.d;
    a.R = W.r.d; a.flags = W.flags.d; a.tol = tol;
    a.res_part = W.res_part.d; a.n_rblocks = W.n_rblocks;
    a.gram_part = W.gram_part.d; a.n_gram_wgs = W.n_gram_wgs; a.n_row_tiles = W.n_row_tiles;
    a.out = W.out.d; a.coef = W.coef.d;
    MvArgs m{};
    m.ptr = be.Kset.mat.ptr.d; m.col = be.Kset.mat.col.d; m.val = op.product_values(R, sigma);
    m.tiles = W.tiles; m.n_tiles = W.n_tiles; m.n = n; m.flags = W.flags.d; m.all_columns = 1; m.pw_part = W.pw_part.d;
    auto product = [&](const double* in, double* out) {
        m.p_in = in; m.w = out;
        hipLaunchKernelGGL(k_mv_product<kSpBlock>, dim3((unsigned)W.n_tiles), dim3(kMvThreads), 0, st, m);
    };
    auto precondition = [&]() {  // W = M^-1 R
        be.precondition_block(W.r.d, W.w.d, W.p_scratch.d, W.aw.d, kSpBlock, n, W.flags.d + kSpBlock, W.rz.d, W.zb.d);
    };
    const dim3 g16((unsigned)W.n_rblocks, (unsigned)kSpBlock), g2((unsigned)W.n_rblocks, 2u), blk(kMvThreads);
    auto gram = [&]() {
        hipLaunchKernelGGL(k_sp_gram, dim3((unsigned)W.n_gram_wgs), blk, 0, st, a);
        hipLaunchKernelGGL(k_sp_gram_sum, dim3((unsigned)((kSpGramOut + kMvThreads - 1) / kMvThreads)), blk, 0, st, a);
    };
    std::vector<double> host((size_t)kSpGramOut + kSpBlock), coef((size_t)kSpM * kSpBlock);
    SpTheta th{};
    double* norms = host.data() + kSpGramOut;
    int kept = 0;
    auto ritz_and_combine = [&]() -> bool {  // false: breakdown
        SpTheta next{};
        const int status = sp_rayleigh_ritz(kSpM, kSpBlock, host.data(), host.data() + kSpM * kSpM, next.v, coef.data(), &kept, Op::indefinite);
        if (status == kSpRrBreakdown) return false;  // (X and its values stay as they are)
        th = next;
        staged_h2d(W.coef.d, coef.data(), coef.size() * sizeof(double), st);
        hipLaunchKernelGGL(k_sp_combine, g2, blk, 0, st, a);
        return true;
    };
    auto residual = [&]() {
        hipLaunchKernelGGL(k_sp_residual, g16, blk, 0, st, a, th);
        hipLaunchKernelGGL(k_sp_done, dim3(1), dim3(kThreads), 0, st, a);
    };
    auto first_k_done = [&]() {
        for (int c = 0; c < k; ++c)
            if (!(norms[c] <= tol)) return false;
        return true;
    };
    const double t1 = now_ms();
    // the start block, orthonormalised by the Gram and combine kernels with W and P out of use
    hipLaunchKernelGGL(k_sp_start, g16, blk, 0, st, a);
    product(W.x.d, W.ax.d);
    a.x_only = 1; a.has_p = 0;
    gram();
    HIP_CHECK(hipGetLastError());
    staged_d2h(host.data(), W.out.d, (size_t)kSpGramOut * sizeof(double), st);
    bool broke = !ritz_and_combine();
    a.x_only = 0;
    int iterations = 0;
    bool final_ready = false;
    while (!broke && iterations < max_iters) {
        residual();
        precondition();
        product(W.w.d, W.aw.d);
        gram();
        HIP_CHECK(hipGetLastError());
        staged_d2h(host.data(), W.out.d, host.size() * sizeof(double), st);  // the one read of the iteration
        if (first_k_done()) {  // ... by the recurrence's AX: look again with the product
            product(W.x.d, W.ax.d);
            residual();
            HIP_CHECK(hipGetLastError());
            staged_d2h(norms, W.out.d + kSpGramOut, (size_t)kSpBlock * sizeof(double), st);
            if (first_k_done()) { final_ready = true; break; }
            continue;  // AX is exact again; the next pass has columns to work on
        }
        if (!ritz_and_combine()) { broke = true; break; }
        a.has_p = 1;
        ++iterations;
    }
    if (!final_ready) {
        product(W.x.d, W.ax.d);
        residual();
        HIP_CHECK(hipGetLastError());
        staged_d2h(norms, W.out.d + kSpGramOut, (size_t)kSpBlock * sizeof(double), st);
    }
    // ascending; unit 2-norm on the way out (X is orthonormal to the rounding of the combine step)
    std::vector<int> order((size_t)k);
    for (int c = 0; c < k; ++c) order[(size_t)c] = c;
    std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return th.v[p] < th.v[q]; });
    std::vector<double> X;
    if (vectors) {
        X.resize((size_t)k * (size_t)n);
        staged_d2h(X.data(), W.x.d, X.size() * sizeof(double), st);
    }
    auto product_with = [&](const double* val, const double* in, double* out) {
        m.val = val;
        product(in, out);
    };
    op.after_iteration(R, product_with, sigma);
    HIP_CHECK(sync_stream(st));
    int unconverged = 0;
    double worst = 0.0;
    for (int j = 0; j < k; ++j) {
        const int c = order[(size_t)j];
        const double rho = norms[c];
        if (!(rho <= tol)) ++unconverged;
        worst = std::isfinite(rho) ? std::max(worst, rho) : INFINITY;
        if (values) values[j] = th.v[c] - sigma;
        if (residuals) residuals[j] = rho;
        if (vectors) {
            const double* src = X.data() + (size_t)c * (size_t)n;
            double* dst = vectors + (size_t)j * (size_t)n;
            long double s = 0.0L;
            for (long long i = 0; i < n; ++i) s += (long double)src[i] * (long double)src[i];
            const double inv = s > 0.0L && std::isfinite((double)s) ? (double)(1.0L / sqrtl(s)) : 1.0;
            for (long long i = 0; i < n; ++i) dst[i] = src[i] * inv;
        }
    }
    const double t2 = now_ms();
    outcome.iterations = iterations; outcome.unconverged = unconverged;
    for (int j = 0; j < k; ++j) outcome.column[j] = order[(size_t)j];
    outcome.h_max = h_max; outcome.sigma = sigma; outcome.worst = worst;
    outcome.setup_ms = t1 - t0; outcome.solve_ms = t2 - t1;
    return unconverged ? 1 : 0;
}

template <class Refine>
int sp_solve(Refine& R, const double* poses, const double* landmarks, int32_t k, double rel_tol, int32_t max_iters, double shift_rel,
             double* values, double* vectors, double* residuals, score_spectrum_info* info) {
    SpInformation op;
    SpOutcome o;
    const int rc = sp_iterate(R, op, poses, landmarks, k, rel_tol, max_iters, shift_rel, values, vectors, residuals, o);
    if (info) {
        info->modes = k; info->block = kSpBlock; info->iterations = o.iterations; info->unconverged = o.unconverged;
        info->h_max = o.h_max; info->shift = o.sigma; info->max_residual = o.worst;
        info->setup_ms = o.setup_ms; info->solve_ms = o.solve_ms;
    }
    return rc;
}

}  // namespace score

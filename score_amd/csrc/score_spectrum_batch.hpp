// score_spectrum_batch.hpp -- the lowest eigenpairs of H = J'J of every member of a refinement group
// (include/score_spectrum_batch.h): the block eigensolver of score_spectrum.hpp crossed with the
// per-member control of score_gn_batch.hpp (section 12), with the Rayleigh-Ritz step on the device (section 16).
//
// What exists already and is used as it is: the blocks of all members (k_gb_blocks<DIM>), the gather of H on the union
// pattern with one shift per member (k_gb_gather_h), one chain factorisation for all members (derive_rho_data), M^-1 on 16
// union vectors in one launch (HipBackend::precondition_block) and the product of one tile over 16 vectors
// (mv_product_tile<16>).  The six blocks X, W, P and AX, AW, AP are U.n x 16 each, column c at c * U.n, plus the residual
// block R and the chain kernel's scratch: 8 buffers x 16 x 8 bytes per unknown of the group, about 0.8 GB at 64 worlds of
// 12 000 unknowns.  They are device allocations of the handle's own, come with the first call and go with the handle.
//
// Every workgroup of every kernel belongs to one member -- found from ublk_member[], tiles[].w, the Gram pass's own table
// or blockIdx -- and tests the member's control word first (mode | has_p << 8, written by the host once per round; the
// modes and the rule that moves a member between them: score_spectrum_batch_rule.hpp).  No reduction crosses a member
// boundary, the number and order of a member's partials depend on n_g alone, and there are no atomics: a member's results
// do not depend on the group around it, and two calls give the same bits.
//   k_gsp_start     the start block from sp_start_value of (member-local unknown, column)
//   k_gsp_hmax      per-workgroup maxima of diag H_g (from the gathered matrix; the host joins a member's own workgroups)
//   k_gsp_product   a verifying member: AX = A X on all 16 columns; an iterating one: AW = A W on its live columns
//   k_gsp_residual  R_c = AX_c - theta_c X_c, per-workgroup partials of |R_c|^2 (theta stays on the device)
//   k_gsp_done      one workgroup per member: the partials of [ublk0, ublk1) re-reduced in order, the done words
//   k_gsp_gram      S'AS and S'S from one pass over the member's rows of the six blocks: sp_gram_tile and sp_gram_store of
//                   score_spectrum.hpp (32 rows x 96 columns, column-major, leading dimension 33) on the directions of
//                   sp_active_mask, kGspGramTiles tiles per workgroup, never across a member
//   k_gsp_gram_sum  the member's partial matrices summed in workgroup order; both matrices stay on the device
//   k_gsp_ritz      Rayleigh-Ritz on the member's pencil, one workgroup per member (below)
//   k_gsp_combine   k_sp_combine's form with the member's own C, broadcast from LDS (the row's text stands in both kernels:
//                   see k_sp_combine)
//
// k_gsp_ritz runs steps 1 to 5 of score_spectrum_rr.hpp, unchanged in meaning, with its thresholds.  The two
// eigen-decompositions are Jacobi with a parallel ordering: a round-robin tournament over the m directions in use (m - 1
// steps of m / 2 disjoint pairs for even m -- 47 steps of 24 pairs at m = 48 --, one more seat that sits out where m is
// odd).  All rotation angles of a step are computed from the matrix as it stands before the step; then the columns of all
// pairs are rotated (the matrix and the accumulated vectors), a barrier, the rows, a barrier.  Disjoint pairs touch
// disjoint columns, then disjoint rows, so the result is that of applying the step's rotations one after the other.
// A wavefront owns six of the step's pairs: six of its lanes compute their angles, shuffles hand them to the other lanes,
// and lane k rotates row k (then column k) of all six, the twelve LDS reads of a pass independent of one another.
// Stopping rule of the host routine: off <= 1e-34 diag, at most 60 sweeps.  The order is fixed: two calls give the same bits.
// LDS: a 48 x 48 double matrix with leading dimension 49 (a column walk then steps 98 banks: 32 distinct even banks per
// half wavefront) is 18.4 KB.  THREE are live at once -- Jacobi's matrix and its vectors, and Y = Q L^-1/2 across the
// second decomposition; the unscaled pencil is re-read from global memory (18 KB each, in L2) when the Rayleigh quotients
// are formed -- plus the 48 x 16 coefficients and the small vectors: 63 KB of static LDS, under the 64 KB a kernel may
// declare (CDNA4 has 160 KiB per CU: two such workgroups fit, and a group launches one per member).
// It writes theta[g][16], C[g][48][16], status[g] and kept[g] with plain vector stores.  GspRitzArgs::indefinite lifts the test
// that the lowest value is positive, as the host routine's argument does, for the pencils of score_curvature_batch.hpp.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/score_spectrum_batch.h"
#include "score_group_pcg.hpp"
#include "score_spectrum.hpp"
#include "score_spectrum_batch_rule.hpp"

namespace score {

static_assert(kGspRitzBreakdown == kSpRrBreakdown, "the rule and the Rayleigh-Ritz routine name breakdown alike");

constexpr int kGspGramTiles = 16;     // row tiles of kSpRows rows per workgroup of the Gram pass
constexpr int kGspLd = kSpM + 1;      // leading dimension of a 48 x 48 matrix in k_gsp_ritz's LDS
constexpr int kGspPairs = kSpM / 2;   // disjoint pairs of a tournament step at most
constexpr int kGspPairsPerWave = kGspPairs / (kThreads / 64);  // ... of which each wavefront of k_gsp_ritz rotates 6
static_assert(kGspPairsPerWave * (kThreads / 64) == kGspPairs && kSpM <= 64, "one lane per row, the pairs dealt evenly");

struct GspArgs {
    GbDev d;
    const int32_t* ptr; const int32_t* col; const double* val;   // A on the union pattern
    const int4* tiles;                                           // {first row, end row, long row?, member}
    int n_tiles, n_ublocks;
    long long n;               // unknowns of the union: the stride of the vectors
    double* S[3];              // X, W, P
    double* AS[3];             // AX, AW, AP
    double* R;
    const int32_t* ctl;        // [g] mode | has_p << 8
    int32_t* flags;            // [g * 16 + c] done word of (member, column)
    int x_only;                // the start: every member forms A X and orthonormalises X, W and P out of use
    int only;                  // product: the mode whose members this launch serves
    const double* tol;         // [g] rel_tol * h_max_g
    double* theta;             // [g * 16 + c]
    double* res_part;          // [c * n_ublocks + workgroup]
    double* norms;             // [g * 16 + c]
    const int4* gram_wgs;      // Gram pass: {member, first row (member-local), row tiles, 0} per workgroup
    const int2* gram_range;    // [g] its workgroups [x, y) of the Gram pass
    double* gram_part;         // [workgroup][2][48][48]
    double* gram;              // [g][2][48][48] S'AS, S'S
    double* coef;              // [g][48][16]
    int32_t* status;           // [g] of the member's last Rayleigh-Ritz step
    int32_t* kept;             // [g]
    double* pw_part;           // the product's partials of p'w (written, not read)
};

__device__ __forceinline__ int gsp_mode(const GspArgs& a, int g) { return a.ctl[g] & 0xff; }

// the directions of member g's S in use (sp_active_mask on the member's words)
__device__ __forceinline__ unsigned long long gsp_active(const GspArgs& a, int g) {
    return sp_active_mask(a.x_only, a.ctl[g] >> 8 & 1, a.flags + g * kSpBlock);
}

// grid (unknown workgroups, 16): the start block, keyed by (member-local unknown, column); the member's done words cleared
__global__ __launch_bounds__(kThreads) void k_gsp_start(GspArgs a) {
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y;
    const GbMember M = a.d.members[g];
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + threadIdx.x;
    if (li < M.n) a.S[0][c * a.n + M.col0 + li] = sp_start_value(li, c);
    if ((int)blockIdx.x == M.ublk0 && threadIdx.x == 0) {
        a.flags[g * kSpBlock + c] = 0;
        a.theta[g * kSpBlock + c] = 0.0;
    }
}

// grid (unknown workgroups): per-workgroup maxima of the diagonal of the gathered matrix (k0: the values k_gb_gather_h
// wrote, on the union pattern; a row's diagonal entry is the one diag_member marks)
__global__ __launch_bounds__(kThreads) void k_gsp_hmax(GspArgs a, const double* __restrict__ k0, const int32_t* __restrict__ diag_member,
                                                       double* __restrict__ part) {
    __shared__ double red[4];
    const int g = a.d.ublk_member[blockIdx.x];
    const GbMember M = a.d.members[g];
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + threadIdx.x;
    double v = 0.0;
    if (li < M.n) {
        const long long row = M.col0 + li;
        for (int k = a.ptr[row]; k < a.ptr[row + 1]; ++k)
            if (diag_member[k]) v = k0[k] == k0[k] ? k0[k] : INFINITY;  // (fmax would drop a NaN)
    }
    v = block_max(v, red);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// grid (tiles): the product of the tile's member, where the member is in mode `only` (the start: every member) -- verifying
// (or starting): AX = A X on all 16 columns; iterating: AW = A W on the live columns
__global__ __launch_bounds__(kThreads) void k_gsp_product(GspArgs a) {
    __shared__ double red[(kThreads / 64) * kSpBlock];
    const int4 tile = a.tiles[blockIdx.x];
    const int g = tile.w;
    bool whole = a.x_only != 0;
    if (!whole) {
        const int mode = gsp_mode(a, g);
        if (mode != a.only) return;
        whole = mode == kGspVerify;
    }
    unsigned live = 0xFFFFu;
    if (!whole) {
        live = 0;
#pragma unroll
        for (int c = 0; c < kSpBlock; ++c)
            if (a.flags[g * kSpBlock + c] == 0) live |= 1u << c;
        if (!live) return;
    }
    mv_product_tile<kSpBlock>(a.ptr, a.col, a.val, tile, a.n, whole ? a.S[0] : a.S[1], whole ? a.AS[0] : a.AS[1], a.pw_part,
                              (size_t)a.n_tiles, (size_t)blockIdx.x, live, red);
}

// grid (unknown workgroups, 16): R_c = AX_c - theta_c X_c on the iterating and the verifying members, partials of |R_c|^2
__global__ __launch_bounds__(kThreads) void k_gsp_residual(GspArgs a) {
    __shared__ double red[4];
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y;
    const int mode = gsp_mode(a, g);
    if (mode != kGspIterate && mode != kGspVerify) return;
    const GbMember M = a.d.members[g];
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + threadIdx.x;
    double dv = 0.0;
    if (li < M.n) {
        const long long e = c * a.n + M.col0 + li;
        dv = a.AS[0][e] - a.theta[g * kSpBlock + c] * a.S[0][e];
        a.R[e] = dv;
    }
    const double s = block_sum(dv * dv, red);
    if (threadIdx.x == 0) a.res_part[(size_t)c * (size_t)a.n_ublocks + blockIdx.x] = s;
}

// grid (members): the member's norms from its own partials [ublk0, ublk1) in a fixed order, its done words
__global__ __launch_bounds__(kThreads) void k_gsp_done(GspArgs a) {
    __shared__ double red[4];
    const int g = blockIdx.x;
    const int mode = gsp_mode(a, g);
    if (mode != kGspIterate && mode != kGspVerify) return;
    const GbMember M = a.d.members[g];
    const double tol = a.tol[g];
    for (int c = 0; c < kSpBlock; ++c) {
        const double s = reduce_partials(a.res_part + (size_t)c * (size_t)a.n_ublocks, M.ublk0, M.ublk1, red);
        if (threadIdx.x == 0) {
            const double nrm = sqrt(s);
            a.norms[g * kSpBlock + c] = nrm;
            a.flags[g * kSpBlock + c] = nrm <= tol ? 1 : 0;  // (a non-finite norm is not done)
        }
    }
}

// grid (Gram workgroups): S'AS and S'S of the member's directions in use over the workgroup's row tiles (sp_gram_tile on
// the member's rows, the workgroup's wg.z tiles one after the other)
__global__ __launch_bounds__(kThreads) void k_gsp_gram(GspArgs a) {
    static_assert(kThreads == kMvThreads, "the Gram tile's thread layout is the single graph's");
    __shared__ double s[kSpM * kSpLd], as[kSpM * kSpLd];
    const int4 wg = a.gram_wgs[blockIdx.x];
    const int g = wg.x;
    if (!a.x_only && gsp_mode(a, g) != kGspIterate) return;
    const GbMember M = a.d.members[g];
    const unsigned long long act = gsp_active(a, g);
    double ga[3][3] = {}, gb[3][3] = {};
    for (int tile = 0; tile < wg.z; ++tile)
        sp_gram_tile(a.S, a.AS, a.n, M.col0, (long long)wg.y + (long long)tile * kSpRows, M.n, act, s, as, ga, gb);
    sp_gram_store(a.gram_part + (size_t)blockIdx.x * (size_t)kSpGramOut, ga, gb);
}

// grid (kSpGramOut / 256, members): the member's partial matrices summed in workgroup order
__global__ __launch_bounds__(kThreads) void k_gsp_gram_sum(GspArgs a) {
    const int g = blockIdx.y;
    if (!a.x_only && gsp_mode(a, g) != kGspIterate) return;
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= kSpGramOut) return;
    const int2 range = a.gram_range[g];
    double acc = 0.0;
    for (int w = range.x; w < range.y; ++w) acc += a.gram_part[(size_t)w * (size_t)kSpGramOut + (size_t)e];
    a.gram[(size_t)g * (size_t)kSpGramOut + (size_t)e] = acc;
}

// ---------------------------------------------------------------------------
// Rayleigh-Ritz on the device
// ---------------------------------------------------------------------------
struct GspRitzLds {
    double m0[kSpM * kGspLd], m1[kSpM * kGspLd], m2[kSpM * kGspLd];
    double c[kSpM * kSpBlock];                        // the coefficients of the directions in use, before the last scaling
    double ev[kSpM], raw[kSpM], d[kSpM], th[kSpBlock], sc[kSpBlock];
    double red[8];
    int idx[kSpM], perm[kSpM];
    int ma, first;
};
static_assert(sizeof(GspRitzLds) <= 64 * 1024, "k_gsp_ritz stays under the static LDS a kernel may declare");

__device__ __forceinline__ bool gsp_finite(double v) { return fabs(v) <= 1.79769313486231570e308; }

// Eigen-decomposition of the symmetric mm x mm matrix a (leading dimension kGspLd, destroyed) by Jacobi in the tournament
// ordering; v: scratch of the same size.  On return ev holds the values ascending and a the vectors as its COLUMNS, in that
// order.  Every lane of the workgroup enters; the result is the same in all of them.  false: an entry is not finite.
__device__ __forceinline__ bool gsp_jacobi(int mm, double* a, double* v, GspRitzLds& L) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double bad = 0.0;
    for (int e = t; e < mm * mm; e += kThreads) {
        const int i = e / mm, j = e % mm;
        v[i * kGspLd + j] = i == j ? 1.0 : 0.0;
        if (!gsp_finite(a[i * kGspLd + j])) bad = 1.0;
    }
    if (block_sum(bad, L.red) != 0.0) return false;
    const int seats = mm + (mm & 1), pairs = seats / 2;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int e = t; e < mm * mm; e += kThreads) {
            const int i = e / mm, j = e % mm;
            const double x = a[i * kGspLd + j];
            if (i == j) diag += x * x;
            else if (i < j) off += x * x;
        }
        block_sum2(off, diag, L.red);
        if (off == 0.0 || off <= 1e-34 * diag) break;
        for (int step = 0; step + 1 < seats; ++step) {
            // the angles of the step, from the matrix as it stands: lane j < 6 of wavefront w owns pair w + 4 j, and its
            // wavefront rotates that pair -- the angles reach the other lanes by shuffles, not through LDS.  (Another
            // wavefront's column pass writes columns r, s of ITS pairs only: a[p][q], a[p][p] and a[q][q] are not among them.)
            int mp = -1, mq = 0;
            double mc = 1.0, ms = 0.0;
            const int pr = wave + 4 * lane;
            if (lane < kGspPairsPerWave && pr < pairs) {
                int p = pr == 0 ? step : (step + pr) % (seats - 1);
                int q = pr == 0 ? seats - 1 : (step - pr + (seats - 1)) % (seats - 1);
                if (p > q) { const int u = p; p = q; q = u; }
                bool on = q < mm;  // (the last seat is empty where mm is odd: its partner sits out)
                if (on) {
                    const double apq = a[p * kGspLd + q];
                    if (apq == 0.0) {
                        on = false;
                    } else {
                        const double app = a[p * kGspLd + p], aqq = a[q * kGspLd + q];
                        if (!(fabs(apq) <= 1e-300 || fabs(apq) < 1e-20 * sqrt(fabs(app) * fabs(aqq)))) {
                            const double tau = (aqq - app) / (2.0 * apq);
                            const double tn = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                            mc = 1.0 / sqrt(1.0 + tn * tn);
                            ms = tn * mc;
                        }  // (else: the entry is rounding; it is set to zero, no rotation)
                    }
                }
                mp = on ? p : -1; mq = q;
            }
            int P[kGspPairsPerWave], Q[kGspPairsPerWave];
            double C[kGspPairsPerWave], S[kGspPairsPerWave];
#pragma unroll
            for (int j = 0; j < kGspPairsPerWave; ++j) {
                P[j] = __shfl(mp, j, 64); Q[j] = __shfl(mq, j, 64);
                C[j] = __shfl(mc, j, 64); S[j] = __shfl(ms, j, 64);
            }
            const int k = lane;  // the row (then the column) this lane rotates, for each of its wavefront's pairs
#pragma unroll
            for (int j = 0; j < kGspPairsPerWave; ++j) {  // columns p, q of the matrix and of the vectors
                if (P[j] < 0 || k >= mm) continue;
                const int p = P[j], q = Q[j];
                const double c = C[j], s = S[j];
                const double akp = a[k * kGspLd + p], akq = a[k * kGspLd + q];
                const double vkp = v[k * kGspLd + p], vkq = v[k * kGspLd + q];
                a[k * kGspLd + p] = c * akp - s * akq;
                a[k * kGspLd + q] = s * akp + c * akq;
                v[k * kGspLd + p] = c * vkp - s * vkq;
                v[k * kGspLd + q] = s * vkp + c * vkq;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < kGspPairsPerWave; ++j) {  // rows p, q; the rotated entry is zero by construction
                if (P[j] < 0 || k >= mm) continue;
                const int p = P[j], q = Q[j];
                const double c = C[j], s = S[j];
                const double apk = a[p * kGspLd + k], aqk = a[q * kGspLd + k];
                a[p * kGspLd + k] = k == q ? 0.0 : c * apk - s * aqk;
                a[q * kGspLd + k] = k == p ? 0.0 : s * apk + c * aqk;
            }
            __syncthreads();
        }
    }
    bad = 0.0;
    if (t < mm) {
        L.raw[t] = a[t * kGspLd + t];
        if (!gsp_finite(L.raw[t])) bad = 1.0;
    }
    if (block_sum(bad, L.red) != 0.0) return false;
    if (t < mm) {  // ascending, by rank (ties in index order); the columns follow
        const double wi = L.raw[t];
        int r = 0;
        for (int j = 0; j < mm; ++j) {
            const double wj = L.raw[j];
            if (wj < wi || (wj == wi && j < t)) ++r;
        }
        L.perm[t] = r;
        L.ev[r] = wi;
    }
    __syncthreads();
    for (int e = t; e < mm * mm; e += kThreads) {
        const int k = e / mm, i = e % mm;
        a[k * kGspLd + L.perm[i]] = v[k * kGspLd + i];
    }
    __syncthreads();
    return true;
}

// One attempt on the pencil (GA, GB), 48 x 48 row-major in global memory, with or without the P block.  true: L.th holds
// the 16 values, L.c * L.sc the coefficients of the directions L.idx[0 .. L.ma).  kept: directions left after step 3.
// indefinite: the pencil of an indefinite A (score_curvature_batch.hpp) -- lifts the test of the lowest value, nothing else.
__device__ __forceinline__ bool gsp_ritz_attempt(const double* __restrict__ GA, const double* __restrict__ GB, bool use_p, bool indefinite,
                                                 GspRitzLds& L, int* kept) {
    const int t = threadIdx.x;
    constexpr int nb = kSpBlock;
    __syncthreads();  // (a second attempt: the first one's reads of L are over)
    if (t == 0) {     // steps 1 and 2: the directions in use and their scales
        int ma = 0;
        for (int i = 0; i < (use_p ? kSpM : 2 * nb); ++i) {
            const double b = GB[i * kSpM + i];
            if (gsp_finite(b) && b > 0.0) { L.idx[ma] = i; L.d[ma] = 1.0 / sqrt(b); ++ma; }
        }
        L.ma = ma;
    }
    __syncthreads();
    const int ma = L.ma;
    *kept = 0;
    if (ma < nb) return false;
    for (int e = t; e < ma * ma; e += kThreads) {
        const int i = e / ma, j = e % ma, gi = L.idx[i], gj = L.idx[j];
        L.m0[i * kGspLd + j] = 0.5 * (GB[gi * kSpM + gj] + GB[gj * kSpM + gi]) * L.d[i] * L.d[j];
    }
    __syncthreads();
    if (!gsp_jacobi(ma, L.m0, L.m1, L)) return false;  // step 3: m0 = Q, ev = L
    const double lmax = L.ev[ma - 1];
    if (!(lmax > 0.0)) return false;
    if (t == 0) {
        int first = 0;
        while (first < ma && !(L.ev[first] > kSpRrDrop * lmax)) ++first;
        L.first = first;
    }
    __syncthreads();
    const int first = L.first, mk = ma - first;
    *kept = mk;
    if (mk < nb) return false;
    for (int e = t; e < ma * mk; e += kThreads) {  // m1 = Y = Q[:, first:] L^-1/2
        const int i = e / mk, j = e % mk;
        L.m1[i * kGspLd + j] = L.m0[i * kGspLd + first + j] / sqrt(L.ev[first + j]);
    }
    __syncthreads();
    for (int e = t; e < ma * ma; e += kThreads) {  // m0 = As, the scaled S'AS
        const int i = e / ma, j = e % ma, gi = L.idx[i], gj = L.idx[j];
        L.m0[i * kGspLd + j] = 0.5 * (GA[gi * kSpM + gj] + GA[gj * kSpM + gi]) * L.d[i] * L.d[j];
    }
    __syncthreads();
    for (int e = t; e < ma * mk; e += kThreads) {  // m2 = As Y
        const int i = e / mk, j = e % mk;
        double s = 0.0;
        for (int k = 0; k < ma; ++k) s += L.m0[i * kGspLd + k] * L.m1[k * kGspLd + j];
        L.m2[i * kGspLd + j] = s;
    }
    __syncthreads();
    for (int e = t; e < mk * mk; e += kThreads) {  // step 4: m0 = T = Y' As Y, the upper triangle mirrored
        const int i = e / mk, j = e % mk;
        if (i > j) continue;
        double s = 0.0;
        for (int k = 0; k < ma; ++k) s += L.m1[k * kGspLd + i] * L.m2[k * kGspLd + j];
        L.m0[i * kGspLd + j] = s;
        L.m0[j * kGspLd + i] = s;
    }
    __syncthreads();
    if (!gsp_jacobi(mk, L.m0, L.m2, L)) return false;  // m0 = Z, ev = mu
    if (!indefinite && !(L.ev[0] > 0.0)) return false;
    for (int e = t; e < ma * nb; e += kThreads) {  // c = D Y Z[:, :nb]
        const int i = e / nb, j = e % nb;
        double s = 0.0;
        for (int k = 0; k < mk; ++k) s += L.m1[i * kGspLd + k] * L.m0[k * kGspLd + j];
        L.c[i * nb + j] = s * L.d[i];
    }
    __syncthreads();
    for (int e = t; e < ma * ma; e += kThreads) {  // m1, m2 = the unscaled pencil on the directions in use
        const int i = e / ma, j = e % ma, gi = L.idx[i], gj = L.idx[j];
        L.m1[i * kGspLd + j] = 0.5 * (GA[gi * kSpM + gj] + GA[gj * kSpM + gi]);
        L.m2[i * kGspLd + j] = 0.5 * (GB[gi * kSpM + gj] + GB[gj * kSpM + gi]);
    }
    __syncthreads();
    for (int e = t; e < ma * nb; e += kThreads) {  // m0 = [B0 c | A0 c]
        const int i = e / nb, j = e % nb;
        double sb = 0.0, sa = 0.0;
        for (int k = 0; k < ma; ++k) {
            const double ck = L.c[k * nb + j];
            sb += L.m2[i * kGspLd + k] * ck;
            sa += L.m1[i * kGspLd + k] * ck;
        }
        L.m0[i * kGspLd + j] = sb;
        L.m0[i * kGspLd + nb + j] = sa;
    }
    __syncthreads();
    double bad = 0.0;
    if (t < nb) {  // c'Bc = 1, theta = c'Ac / c'Bc of the unscaled matrices
        double cbc = 0.0, cac = 0.0;
        for (int i = 0; i < ma; ++i) {
            cbc += L.c[i * nb + t] * L.m0[i * kGspLd + t];
            cac += L.c[i * nb + t] * L.m0[i * kGspLd + nb + t];
        }
        if (!(cbc > 0.0) || !gsp_finite(cbc) || !gsp_finite(cac)) bad = 1.0;
        L.sc[t] = 1.0 / sqrt(cbc);
        L.th[t] = cac / cbc;
    }
    return block_sum(bad, L.red) == 0.0;
}

struct GspRitzArgs {
    const int32_t* ctl;    // null: every pencil (score_spectrum_ritz)
    const double* GA;      // pencil g: GA + g * ga_stride, GB + g * ga_stride
    const double* GB;
    long long stride;
    double* theta; double* coef; int32_t* status; int32_t* kept;
    int32_t indefinite;    // non-zero: A may be indefinite (gsp_ritz_attempt)
};

// grid (members): the 16 lowest Ritz pairs of the member's pencil (the head of the file); a pencil that breaks down leaves
// theta and C as they were
__global__ __launch_bounds__(kThreads) void k_gsp_ritz(GspRitzArgs a) {
    __shared__ GspRitzLds L;
    const int g = blockIdx.x, t = threadIdx.x;
    if (a.ctl && (a.ctl[g] & 0xff) != kGspIterate) return;
    const double* GA = a.GA + (size_t)g * (size_t)a.stride;
    const double* GB = a.GB + (size_t)g * (size_t)a.stride;
    int kept = 0, status = kSpRrBreakdown;
#pragma unroll 1
    for (int attempt = 0; attempt < 2; ++attempt)  // step 5: once more without the P block (kSpRrOk = 0, kSpRrNoP = 1)
        if (gsp_ritz_attempt(GA, GB, attempt == 0, a.indefinite != 0, L, &kept)) { status = attempt; break; }
    if (status != kSpRrBreakdown) {
        if (t < kSpM) L.perm[t] = -1;  // where direction t sits among those in use
        __syncthreads();
        if (t < L.ma) L.perm[L.idx[t]] = t;
        __syncthreads();
        for (int e = t; e < kSpM * kSpBlock; e += kThreads) {
            const int i = L.perm[e / kSpBlock], j = e % kSpBlock;
            a.coef[(size_t)g * (size_t)(kSpM * kSpBlock) + (size_t)e] = i >= 0 ? L.c[i * kSpBlock + j] * L.sc[j] : 0.0;
        }
        if (t < kSpBlock) a.theta[g * kSpBlock + t] = L.th[t];
    }
    if (t == 0) { a.status[g] = status; a.kept[g] = kept; }
}

// grid (unknown workgroups, 2), one row per lane, on the iterating members whose Rayleigh-Ritz step did not break down:
// y = 0: X <- S C, P <- [W | P] C_wp; y = 1: the same combination of AS into AX, AP.  A lane reads its row of all three
// blocks before it writes: in place.
__global__ __launch_bounds__(kThreads) void k_gsp_combine(GspArgs a) {
    __shared__ double c[kSpM * kSpBlock];
    const int g = a.d.ublk_member[blockIdx.x];
    if (!a.x_only && gsp_mode(a, g) != kGspIterate) return;
    if (a.status[g] == kSpRrBreakdown) return;
    for (int e = threadIdx.x; e < kSpM * kSpBlock; e += kThreads) c[e] = a.coef[(size_t)g * (size_t)(kSpM * kSpBlock) + (size_t)e];
    __syncthreads();
    const unsigned long long act = gsp_active(a, g);
    const GbMember M = a.d.members[g];
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + threadIdx.x;
    if (li >= M.n) return;
    const long long i = M.col0 + li;
    double* const* blk = blockIdx.y ? a.AS : a.S;
    double x[kSpBlock], p[kSpBlock];
#pragma unroll
    for (int j = 0; j < kSpBlock; ++j) x[j] = p[j] = 0.0;
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

// The solver's buffers: device allocations of their own (not the handle's arena); they come with the first call and go
// with the handle (the figure at the head of the file).
struct GspWork {
    DevBuf<double> x, w, p, ax, aw, ap, r, scratch, pw_part, rz, zb, res_part, gram_part, gram, coef, theta, norms, tol, hmax_part;
    DevBuf<int32_t> ctl, flags, status, kept;  // flags: [g * 16 + c], then a zero (the chain kernel's done word)
    DevBuf<int4> gram_wgs;
    DevBuf<int2> gram_range;
    int n_gram_wgs = 0;
    void reserve(const GbUnion& U, size_t n_tiles, size_t n_ublocks, size_t n_prec, size_t zb_per_vector, hipStream_t st) {
        if (x.d) return;
        NoArena no_arena;
        const size_t nv = (size_t)kSpBlock, n = (size_t)U.n, G = (size_t)U.count;
        // the Gram pass's own table: kGspGramTiles row tiles per workgroup, a member's workgroups from its n alone
        std::vector<int4> wgs;
        std::vector<int2> range;
        for (int g = 0; g < U.count; ++g) {
            const long long tiles = (U.members[(size_t)g].n + kSpRows - 1) / kSpRows;
            const int first = (int)wgs.size();
            for (long long t0 = 0; t0 < tiles; t0 += kGspGramTiles)
                wgs.push_back(make_int4(g, (int)(t0 * kSpRows), (int)std::min<long long>(kGspGramTiles, tiles - t0), 0));
            range.push_back(make_int2(first, (int)wgs.size()));
        }
        n_gram_wgs = (int)wgs.size();
        gram_wgs.alloc(wgs.size()); staged_h2d(gram_wgs.d, wgs.data(), wgs.size() * sizeof(int4), st);
        gram_range.alloc(range.size()); staged_h2d(gram_range.d, range.data(), range.size() * sizeof(int2), st);
        DevBuf<double>* vecs[] = {&x, &w, &p, &ax, &aw, &ap, &r, &scratch};
        for (DevBuf<double>* v : vecs) { v->alloc(nv * n); v->zero(st); }
        pw_part.alloc(nv * n_tiles); pw_part.zero(st);
        rz.alloc(nv * n_prec + 4096); rz.zero(st);  // (every workgroup of a chain-kernel launch has a slot, per vector)
        zb.alloc(nv * std::max<size_t>(1, zb_per_vector)); zb.zero(st);
        res_part.alloc(nv * n_ublocks); res_part.zero(st);
        gram_part.alloc((size_t)n_gram_wgs * (size_t)kSpGramOut); gram_part.zero(st);
        gram.alloc(G * (size_t)kSpGramOut); gram.zero(st);
        coef.alloc(G * (size_t)kSpM * nv); coef.zero(st);
        theta.alloc(G * nv); theta.zero(st);
        norms.alloc(G * nv); norms.zero(st);
        tol.alloc(G); tol.zero(st);
        hmax_part.alloc(n_ublocks); hmax_part.zero(st);
        ctl.alloc(G); ctl.zero(st);
        flags.alloc(G * nv + 1); flags.zero(st);
        status.alloc(G); status.zero(st);
        kept.alloc(G); kept.zero(st);
    }
};

// What a call of the group's iteration is about, as SpInformation / SpCurvature say it for one graph: whose words open its
// messages, the values the product reads (asked for once the members' shifts stand in the handle's `lambda` and the chain
// factors of J'J + sigma_g I are derived; it runs inside the setup), whether A may be indefinite (the Ritz step's test of the
// lowest value), and what follows the rounds while X and the blocks still stand.
// GspInformation: score_refine_batch_spectrum, A_g = J'J + sigma_g I in the handle's own values.  score_curvature_batch.hpp
// has the other.
struct GspInformation {
    static constexpr bool indefinite = false;
    const char* who = "score_refine_batch_spectrum: ";
    template <class Batch>
    const double* product_values(Batch& B) { return B.be().Kset.mat.val.d; }
    template <class Batch>
    void after_iteration(Batch&, const GspArgs&) {}
};

// what the iteration reports beside its outputs: the fields score_spectrum_batch_info and score_curvature_batch_info share,
// and per member its shift, its values (k, ascending, the shift taken out) and the column of X behind each of them
struct GspOutcome {
    int rounds = 0, unconverged = 0;
    double worst = 0.0, setup_ms = 0.0, solve_ms = 0.0;
    std::vector<double> h_max, sigma, value;
    std::vector<int> column;
};

// The solve, one body for both operators.  Batch: score_refine_batch (its union, point, blocks and gather, its linear-mode
// handle, its GspWork `spb`).  The preconditioner is that of J'J + sigma_g I whatever the product reads.
template <class Batch, class Op>
int gsp_iterate(Batch& B, Op& op, const double* poses, const double* landmarks, int32_t k, double rel_tol, int32_t max_iters,
                double shift_rel, double* values, double* vectors, double* residuals, int32_t* iterations, double* h_max_out,
                GspOutcome& outcome) {
    const GbUnion& U = B.U;
    const char* who = op.who;
    if (k < 1 || k > kSpBlock) throw std::runtime_error(std::string(who) + "k must be 1..16");
    if (!(rel_tol > 0.0) || !std::isfinite(rel_tol) || max_iters < 1)
        throw std::runtime_error(std::string(who) + "rel_tol must be positive and max_iters >= 1");
    if (!(shift_rel > 0.0) || !std::isfinite(shift_rel)) throw std::runtime_error(std::string(who) + "shift_rel must be positive");
    HipBackend& be = B.be();
    hipStream_t st = B.stream();
    const int G = U.count;
    const long long n = U.n;
    if (be.split.active) throw std::runtime_error(std::string(who) + "the block needs the unsplit chain kernel (chain_split = 0)");
    for (int g = 0; g < G; ++g)
        if (U.members[(size_t)g].n < kSpMinN)
            throw std::runtime_error(std::string(who) + "member " + std::to_string(g) + ": " + std::to_string(U.members[(size_t)g].n) +
                                     " unknowns -- fewer than the 48 the basis holds: use the dense solver (engine=\"python\") for a graph this small");
    const double t0 = now_ms();
    auto& W = B.spb;
    W.reserve(U, (size_t)B.n_tiles, (size_t)B.n_ublocks, (size_t)be.n_prec, (size_t)be.H->bs * (size_t)be.n_join_seps, st);

    GspArgs a{};
    a.d = B.dev();
    a.ptr = be.Kset.mat.ptr.d; a.col = be.Kset.mat.col.d; a.val = be.Kset.mat.val.d;
    a.tiles = B.tiles.d; a.n_tiles = B.n_tiles; a.n_ublocks = B.n_ublocks; a.n = n;
    a.S[0] = W.x.d; a.S[1] = W.w.d; a.S[2] = W.p.d;
    a.AS[0] = W.ax.d; a.AS[1] = W.aw.d; a.AS[2] = W.ap.d;
    a.R = W.r.d; a.ctl = W.ctl.d; a.flags = W.flags.d; a.tol = W.tol.d; a.theta = W.theta.d;
    a.res_part = W.res_part.d; a.norms = W.norms.d;
    a.gram_wgs = W.gram_wgs.d; a.gram_range = W.gram_range.d; a.gram_part = W.gram_part.d; a.gram = W.gram.d;
    a.coef = W.coef.d; a.status = W.status.d; a.kept = W.kept.d; a.pw_part = W.pw_part.d;
    GspRitzArgs ra{};
    ra.ctl = W.ctl.d; ra.GA = W.gram.d; ra.GB = W.gram.d + kSpM * kSpM; ra.stride = kSpGramOut;
    ra.theta = W.theta.d; ra.coef = W.coef.d; ra.status = W.status.d; ra.kept = W.kept.d;
    ra.indefinite = Op::indefinite ? 1 : 0;

    // the points, the blocks, max diag H_g; then A_g = H_g + sigma_g I on the union pattern and the chain factors of all members
    B.set_point(poses, landmarks);
    B.eval(std::vector<char>((size_t)G, 1), false, true, nullptr);
    std::vector<double> sigma((size_t)G, 0.0), tol((size_t)G, 0.0), hmax((size_t)G, 0.0);
    B.gather_h(sigma.data());
    const dim3 bt(kThreads);
    hipLaunchKernelGGL(k_gsp_hmax, dim3((unsigned)B.n_ublocks), bt, 0, st, a, (const double*)be.K0d.d, (const int32_t*)B.diag_member.d, W.hmax_part.d);
    HIP_CHECK(hipGetLastError());
    std::vector<double> hpart((size_t)B.n_ublocks);
    staged_d2h(hpart.data(), W.hmax_part.d, hpart.size() * sizeof(double), st);
    for (int g = 0; g < G; ++g) {
        const GbMember& M = U.members[(size_t)g];
        double h = 0.0;
        for (int b = M.ublk0; b < M.ublk1; ++b) h = std::max(h, hpart[(size_t)b]);
        if (!(h > 0.0) || !std::isfinite(h))
            throw std::runtime_error(std::string(who) + "member " + std::to_string(g) + ": the diagonal of H is zero or not finite at this point");
        hmax[(size_t)g] = h; sigma[(size_t)g] = shift_rel * h; tol[(size_t)g] = rel_tol * h;
    }
    B.gather_h(sigma.data());
    be.derive_rho_data(false);
    staged_h2d(W.tol.d, tol.data(), tol.size() * sizeof(double), st);  // (waits for the stream: sigma has been read)
    a.val = op.product_values(B);

    std::vector<GspState> S((size_t)G);
    std::vector<int32_t> words((size_t)G), status((size_t)G, 0);
    std::vector<double> norms((size_t)G * kSpBlock, 0.0);
    auto write_words = [&]() {
        for (int g = 0; g < G; ++g) words[(size_t)g] = gsp_word(S[(size_t)g]);
        staged_h2d(W.ctl.d, words.data(), words.size() * sizeof(int32_t), st);
    };
    auto any_in = [&](GspMode m) { return std::any_of(S.begin(), S.end(), [m](const GspState& s) { return s.mode == m; }); };
    const dim3 gu16((unsigned)B.n_ublocks, (unsigned)kSpBlock), gu2((unsigned)B.n_ublocks, 2u);
    auto product = [&](int only) {
        a.only = only;
        hipLaunchKernelGGL(k_gsp_product, dim3((unsigned)B.n_tiles), bt, 0, st, a);
    };
    auto ritz_and_combine = [&]() {
        hipLaunchKernelGGL(k_gsp_gram, dim3((unsigned)W.n_gram_wgs), bt, 0, st, a);
        hipLaunchKernelGGL(k_gsp_gram_sum, dim3((unsigned)((kSpGramOut + kThreads - 1) / kThreads), (unsigned)G), bt, 0, st, a);
        hipLaunchKernelGGL(k_gsp_ritz, dim3((unsigned)G), bt, 0, st, ra);
        hipLaunchKernelGGL(k_gsp_combine, gu2, bt, 0, st, a);
    };
    const double t1 = now_ms();
    // the start block of every member, orthonormalised by the Gram, Rayleigh-Ritz and combine kernels with W and P out of use
    for (GspState& s : S) gsp_begin(s);
    write_words();
    a.x_only = 1;
    hipLaunchKernelGGL(k_gsp_start, gu16, bt, 0, st, a);
    product(kGspIterate);
    ritz_and_combine();
    a.x_only = 0;
    int rounds = 0;
    for (;;) {
        ++rounds;
        if (any_in(kGspVerify)) product(kGspVerify);
        hipLaunchKernelGGL(k_gsp_residual, gu16, bt, 0, st, a);
        hipLaunchKernelGGL(k_gsp_done, dim3((unsigned)G), bt, 0, st, a);
        HIP_CHECK(hipGetLastError());
        staged_d2h(norms.data(), W.norms.d, norms.size() * sizeof(double), st);  // the read of the round: 17 words per member
        staged_d2h(status.data(), W.status.d, status.size() * sizeof(int32_t), st);
        for (int g = 0; g < G; ++g)
            if (gsp_live(S[(size_t)g]))
                gsp_after_residual(S[(size_t)g], norms.data() + (size_t)g * kSpBlock, k, tol[(size_t)g], status[(size_t)g], max_iters);
        if (!any_in(kGspIterate) && !any_in(kGspVerify)) break;
        write_words();
        if (!any_in(kGspIterate)) continue;
        be.precondition_block(W.r.d, W.w.d, W.scratch.d, W.aw.d, kSpBlock, n, W.flags.d + (size_t)G * kSpBlock, W.rz.d, W.zb.d);  // W = M^-1 R
        product(kGspIterate);
        ritz_and_combine();
    }
    op.after_iteration(B, a);
    // ascending per member; unit 2-norm on the way out (X is orthonormal to the rounding of the combine step)
    std::vector<double> theta((size_t)G * kSpBlock), X;
    staged_d2h(theta.data(), W.theta.d, theta.size() * sizeof(double), st);
    if (vectors) {
        X.resize((size_t)k * (size_t)n);
        staged_d2h(X.data(), W.x.d, X.size() * sizeof(double), st);
    }
    HIP_CHECK(sync_stream(st));
    int unconverged = 0;
    double worst = 0.0;
    size_t vec0 = 0;
    outcome.value.assign((size_t)G * (size_t)k, 0.0); outcome.column.assign((size_t)G * (size_t)k, 0);
    for (int g = 0; g < G; ++g) {
        const GbMember& M = U.members[(size_t)g];
        const GspState& s = S[(size_t)g];
        const double* th = theta.data() + (size_t)g * kSpBlock;
        const double* nr = norms.data() + (size_t)g * kSpBlock;
        std::vector<int> order((size_t)k);
        for (int c = 0; c < k; ++c) order[(size_t)c] = c;
        std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return th[p] < th[q]; });
        if (!s.converged) ++unconverged;
        for (int j = 0; j < k; ++j) {
            const int c = order[(size_t)j];
            const double rho = nr[c];
            worst = std::isfinite(rho) ? std::max(worst, rho) : INFINITY;
            outcome.value[(size_t)g * (size_t)k + (size_t)j] = th[c] - sigma[(size_t)g];
            outcome.column[(size_t)g * (size_t)k + (size_t)j] = c;
            if (values) values[(size_t)g * (size_t)k + (size_t)j] = th[c] - sigma[(size_t)g];
            if (residuals) residuals[(size_t)g * (size_t)k + (size_t)j] = rho;
            if (vectors) {
                const double* src = X.data() + (size_t)c * (size_t)n + (size_t)M.col0;
                double* dst = vectors + vec0 + (size_t)j * (size_t)M.n;
                long double sq = 0.0L;
                for (long long i = 0; i < M.n; ++i) sq += (long double)src[i] * (long double)src[i];
                const double inv = sq > 0.0L && std::isfinite((double)sq) ? (double)(1.0L / sqrtl(sq)) : 1.0;
                for (long long i = 0; i < M.n; ++i) dst[i] = src[i] * inv;
            }
        }
        vec0 += (size_t)k * (size_t)M.n;
        if (iterations) iterations[g] = gsp_reported_iterations(s);
        if (h_max_out) h_max_out[g] = hmax[(size_t)g];
    }
    const double t2 = now_ms();
    outcome.rounds = rounds; outcome.unconverged = unconverged; outcome.worst = worst;
    outcome.setup_ms = t1 - t0; outcome.solve_ms = t2 - t1;
    outcome.h_max = hmax; outcome.sigma = sigma;
    return unconverged ? 1 : 0;
}

template <class Batch>
int gsp_solve(Batch& B, const double* poses, const double* landmarks, int32_t k, double rel_tol, int32_t max_iters, double shift_rel,
              double* values, double* vectors, double* residuals, int32_t* iterations, double* h_max_out, score_spectrum_batch_info* info) {
    GspInformation op;
    GspOutcome o;
    const int rc = gsp_iterate(B, op, poses, landmarks, k, rel_tol, max_iters, shift_rel, values, vectors, residuals, iterations, h_max_out, o);
    if (info) {
        info->members = B.U.count; info->modes = k; info->block = kSpBlock; info->rounds = o.rounds; info->unconverged = o.unconverged;
        info->max_residual = o.worst; info->setup_ms = o.setup_ms; info->solve_ms = o.solve_ms;
    }
    return rc;
}

// score_spectrum_ritz (and, with the indefinite rule, score_curvature_ritz): k_gsp_ritz alone on the caller's pencils, on
// buffers of the call's own
inline void gsp_ritz_alone(int32_t count, const double* GA, const double* GB, double* theta, double* coef, int32_t* status, int32_t* kept,
                           bool indefinite = false, const char* who = "score_spectrum_ritz: ") {
    if (count < 1) throw std::runtime_error(std::string(who) + "count must be positive");
    if (!GA || !GB) throw std::runtime_error(std::string(who) + "the pencils are missing");
    NoArena no_arena;
    hipStream_t st = nullptr;
    const size_t G = (size_t)count, mm = (size_t)kSpM * kSpM;
    DevBuf<double> dA, dB, dth, dc;
    DevBuf<int32_t> dst, dk;
    dA.alloc(G * mm); dB.alloc(G * mm); dth.alloc(G * kSpBlock); dc.alloc(G * kSpM * kSpBlock); dst.alloc(G); dk.alloc(G);
    staged_h2d(dA.d, GA, G * mm * sizeof(double), st);
    staged_h2d(dB.d, GB, G * mm * sizeof(double), st);
    // (a pencil that breaks down leaves its theta and coef as the caller passed them)
    if (theta) staged_h2d(dth.d, theta, G * kSpBlock * sizeof(double), st);
    if (coef) staged_h2d(dc.d, coef, G * kSpM * kSpBlock * sizeof(double), st);
    GspRitzArgs ra{};
    ra.GA = dA.d; ra.GB = dB.d; ra.stride = (long long)mm;
    ra.theta = dth.d; ra.coef = dc.d; ra.status = dst.d; ra.kept = dk.d;
    ra.indefinite = indefinite ? 1 : 0;
    hipLaunchKernelGGL(k_gsp_ritz, dim3((unsigned)count), dim3(kThreads), 0, st, ra);
    HIP_CHECK(hipGetLastError());
    if (theta) staged_d2h(theta, dth.d, G * kSpBlock * sizeof(double), st);
    if (coef) staged_d2h(coef, dc.d, G * kSpM * kSpBlock * sizeof(double), st);
    if (status) staged_d2h(status, dst.d, G * sizeof(int32_t), st);
    if (kept) staged_d2h(kept, dk.d, G * sizeof(int32_t), st);
    HIP_CHECK(sync_stream(st));
}

}  // namespace score

// score_marginals_batch.hpp -- marginal covariances of every member of a refinement group (include/score_marginals_batch.h):
// the block conjugate-gradient iteration of score_marginals.hpp crossed with the per-member control
// of score_gn_batch.hpp (section 12).
//
// H = J'J of the union is block diagonal, so ONE union vector carries one unit column of EVERY member: NV union vectors,
// stored one after the other with stride U.n (the layout PrecArgs::vec_stride expects), advance NV columns of all members in
// one pass over the union matrix.  In pass k of width W, slot c of member g carries that member's column k W + c; a slot with
// k W + c >= C_g gets r = 0 and done word 1 from the start.  NV is chosen per pass: the smallest of 1, 2, 4, 8, 16 that
// holds the most live slots of any member.
//
// What exists already and is used as it is: the blocks of all members (k_gb_blocks<DIM>), the gather of H on the
// union pattern (k_gb_gather_h, lambda = 0), one chain factorisation for all members (derive_rho_data -> k_factor), M^-1 on
// several union vectors in one launch (launch_prec<PREC_INIT> with PrecArgs::n_vec), and the product of one tile
// (mv_product_tile of score_marginals.hpp).  New here: every (member, slot) pair has its own alpha, beta, gate and done word.
//
// Per-slot words: done[g NV + c], iters[g NV + c], ref[g NV + c].  Partials: pw_part[c n_tiles + tile],
// rz_part[c n_ublocks + workgroup].  Every workgroup of the k_gbm_* kernels below belongs to one member -- taken from
// tiles[].w or ublk_member[], exactly as in the k_gb_* kernels -- tests the done word of its (member, slot) first, and leaves
// a done slot's x, r and p as they are.  One iteration:
//   k_gbm_product    w_c = H p_c for the live slots of the tile's member from ONE pass over the union CSR, per-tile partials of p'w
//   k_gbm_step       alpha = r'z / p'w of (member, slot), both re-reduced in fixed order over the member's own partial ranges
//                    [tile0, tile1) and [ublk0, ublk1) at the slot's offset; x += alpha p, r -= alpha w
//   launch_prec      z_c = M^-1 r_c, every slot of the whole group (a done slot's z is scratch)
//   k_gbm_rz         per-workgroup partials of r_c'z_c
//   k_gbm_direction  beta = r'z_new / r'z_old, p = z + beta p; the gate r'z_new <= rel_tol^2 r0'z0 raises the slot's done word
// Done words: 1 converged (or no column), 2 broken down (a non-finite r'z or p'w, or p'w <= 0) -- reported as not converged.
// No atomics: all workgroups of a (member, slot) reduce the same partials in the same order and take the same decision.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/score_marginals_batch.h"
#include "score_gn_batch.hpp"
#include "score_marginals.hpp"

namespace score {

// (the union's tiles are cut by the rule of mv_tiles: mv_product_tile serves both)
static_assert(kThreads == kMvThreads && kGbLanes == kMvLanes && kGbRows == kMvRows && kGbLongRow == kMvLongRow,
              "the group's product tiles must be the tiles of score_marginals.hpp");

struct GbmArgs {
    GbDev d;
    const int32_t* ptr; const int32_t* col; const double* val;   // H on the union pattern
    const int4* tiles;                                           // {first row, end row, long row?, member}
    int n_tiles, n_ublocks;
    long long n;               // unknowns of the union: the stride of the vectors
    int NV;                    // slots of the pass
    int32_t* done;             // [g * NV + c]
    int32_t* iters;            // [g * NV + c] steps executed
    double* ref;               // [g * NV + c] rel_tol^2 r0'z0
    int all_slots;             // product: every slot that holds a column, whatever its done word (the residual's product H x)
    // vectors of the pass, slot c at c * n
    double* x; double* r; const double* z; double* p; double* w;
    const double* p_in;        // the product's operand (p, or x for the residual)
    double* pw_part;           // [c * n_tiles + tile]
    double* rz_part;           // [c * n_ublocks + workgroup]: k_gbm_rz writes
    const double* rz_new;      // partials of the last application of M^-1
    const double* rz_old;
    int first;                 // direction: p = z, the gate's threshold is set
    double tol2;
    // the columns: member g selects the member-local unknowns sel[sel_ptr[g] .. sel_ptr[g + 1])
    const int32_t* sel_ptr; const int32_t* sel;
    const int32_t* sel_member; // [selected row] its member
    const long long* joint_off;  // [g] where the member's C_g x C_g matrix starts in joint
    int n_sel;                 // sum of C_g
    int k0, width;             // the pass: slot c carries column k0 + c, c < width
    double* res_part;          // [c * n_ublocks + workgroup]
    double* joint;
};

// the column slot c of member g carries in this pass (-1: none)
__device__ __forceinline__ int gbm_column(const GbmArgs& a, int g, int c) {
    const int col = a.k0 + c;
    return (c < a.width && col < a.sel_ptr[g + 1] - a.sel_ptr[g]) ? col : -1;
}

// grid (unknown workgroups, NV): x = 0, r = the unit vector of the slot's unknown; the slot's words
__global__ __launch_bounds__(kThreads) void k_gbm_rhs(GbmArgs a) {
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y, t = threadIdx.x;
    const GbMember M = a.d.members[g];
    const int col = gbm_column(a, g, c);
    const long long unit = col >= 0 ? (long long)a.sel[a.sel_ptr[g] + col] : -1;
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + t;
    if (li < M.n) {
        const long long e = c * a.n + M.col0 + li;
        a.x[e] = 0.0;
        a.r[e] = li == unit ? 1.0 : 0.0;
    }
    if ((int)blockIdx.x == M.ublk0 && t == 0) {
        a.done[g * a.NV + c] = col >= 0 ? 0 : 1;
        a.iters[g * a.NV + c] = 0;
        a.ref[g * a.NV + c] = 0.0;
    }
}

// grid (tiles): w_c = H p_in_c over the live slots of the tile's member, per-tile partials of p_in_c'w_c
template <int NV>
__global__ __launch_bounds__(kThreads) void k_gbm_product(GbmArgs a) {
    __shared__ double red[(kThreads / 64) * NV];
    const int4 tile = a.tiles[blockIdx.x];
    const int g = tile.w;
    unsigned live = 0;
#pragma unroll
    for (int c = 0; c < NV; ++c)
        if (a.all_slots ? gbm_column(a, g, c) >= 0 : a.done[g * NV + c] == 0) live |= 1u << c;
    if (!live) return;
    mv_product_tile<NV>(a.ptr, a.col, a.val, tile, a.n, a.p_in, a.w, a.pw_part, (size_t)a.n_tiles, (size_t)blockIdx.x, live, red);
}

// grid (unknown workgroups, NV): alpha = r'z / p'w of (member, slot) ; x += alpha p ; r -= alpha w
__global__ __launch_bounds__(kThreads) void k_gbm_step(GbmArgs a) {
    __shared__ double red[8];
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y, t = threadIdx.x;
    const int word = g * a.NV + c;
    if (a.done[word]) return;
    const GbMember M = a.d.members[g];
    const double* rzp = a.rz_new + (size_t)c * a.n_ublocks;
    const double* pwp = a.pw_part + (size_t)c * a.n_tiles;
    double rz = 0.0, pw = 0.0;
    for (int i = M.ublk0 + t; i < M.ublk1; i += kThreads) rz += rzp[i];
    for (int i = M.tile0 + t; i < M.tile1; i += kThreads) pw += pwp[i];
    block_sum2(rz, pw, red);
    const bool lead = (int)blockIdx.x == M.ublk0 && t == 0;
    if (!(gb_finite(rz) && gb_finite(pw) && pw > 0.0)) {
        if (lead) a.done[word] = 2;
        return;
    }
    const double alpha = rz / pw;
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + t;
    if (li < M.n) {
        const long long e = c * a.n + M.col0 + li;
        a.x[e] += alpha * a.p[e];
        a.r[e] -= alpha * a.w[e];
    }
    if (lead) a.iters[word] += 1;
}

// grid (unknown workgroups, NV): per-workgroup partials of r_c'z_c on the live slots
__global__ __launch_bounds__(kThreads) void k_gbm_rz(GbmArgs a) {
    __shared__ double red[4];
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y, t = threadIdx.x;
    if (a.done[g * a.NV + c]) return;
    const GbMember M = a.d.members[g];
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + t;
    double v = 0.0;
    if (li < M.n) {
        const long long e = c * a.n + M.col0 + li;
        v = a.r[e] * a.z[e];
    }
    const double s = block_sum(v, red);
    if (t == 0) a.rz_part[(size_t)c * a.n_ublocks + blockIdx.x] = s;
}

// grid (unknown workgroups, NV): the gate of (member, slot), then p = z + beta p (first: p = z and the gate's threshold)
__global__ __launch_bounds__(kThreads) void k_gbm_direction(GbmArgs a) {
    __shared__ double red[8];
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y, t = threadIdx.x;
    const int word = g * a.NV + c;
    if (a.done[word]) return;
    const GbMember M = a.d.members[g];
    const double* rn = a.rz_new + (size_t)c * a.n_ublocks;
    const double* ro = a.first ? nullptr : a.rz_old + (size_t)c * a.n_ublocks;
    double rzn = 0.0, rzo = 0.0;
    for (int i = M.ublk0 + t; i < M.ublk1; i += kThreads) {
        rzn += rn[i];
        if (!a.first) rzo += ro[i];
    }
    block_sum2(rzn, rzo, red);
    const bool lead = (int)blockIdx.x == M.ublk0 && t == 0;
    double beta = 0.0;
    if (a.first) {
        if (!(gb_finite(rzn) && rzn > 0.0)) {  // (a zero right-hand side is solved by x = 0; anything else is no SPD preconditioner)
            if (lead) a.done[word] = rzn == 0.0 ? 1 : 2;
            return;
        }
        if (lead) a.ref[word] = a.tol2 * rzn;
    } else {
        if (!(gb_finite(rzn) && rzo > 0.0)) {
            if (lead) a.done[word] = 2;
            return;
        }
        if (rzn <= a.ref[word]) {
            if (lead) a.done[word] = 1;
            return;
        }
        beta = rzn / rzo;
    }
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + t;
    if (li < M.n) {
        const long long e = c * a.n + M.col0 + li;
        a.p[e] = a.first ? a.z[e] : a.z[e] + beta * a.p[e];
    }
}

// grid (unknown workgroups, NV): partials of |e_c - w_c|^2 with w = H x, on the slots that hold a column
__global__ __launch_bounds__(kThreads) void k_gbm_residual(GbmArgs a) {
    __shared__ double red[4];
    const int g = a.d.ublk_member[blockIdx.x], c = blockIdx.y, t = threadIdx.x;
    const int col = gbm_column(a, g, c);
    if (col < 0) return;
    const GbMember M = a.d.members[g];
    const long long unit = a.sel[a.sel_ptr[g] + col];
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + t;
    double dv = 0.0;
    if (li < M.n) dv = (li == unit ? 1.0 : 0.0) - a.w[c * a.n + M.col0 + li];
    const double s = block_sum(dv * dv, red);
    if (t == 0) a.res_part[(size_t)c * a.n_ublocks + blockIdx.x] = s;
}

// grid (blocks over all selected rows, NV): joint_g[s, k0 + c] = x_c[col0_g + sel_g[s]]
__global__ __launch_bounds__(kThreads) void k_gbm_gather(GbmArgs a) {
    const int c = blockIdx.y;
    const long long row = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (row >= a.n_sel) return;
    const int g = a.sel_member[row];
    const int col = gbm_column(a, g, c);
    if (col < 0) return;
    const long long Cg = a.sel_ptr[g + 1] - a.sel_ptr[g], s = row - a.sel_ptr[g];
    a.joint[a.joint_off[g] + s * Cg + col] = a.x[c * a.n + a.d.members[g].col0 + a.sel[row]];
}

// The selected unknowns of every member, member-local, in the order of include/score_marginals.h
inline void gbm_columns(const GbUnion& U, const int32_t* var_ptr, const int32_t* vars, std::vector<int32_t>& sel_ptr,
                        std::vector<int32_t>& sel) {
    if (!var_ptr) throw std::runtime_error("score_refine_batch_marginals: var_ptr is null");
    if (var_ptr[0] != 0) throw std::runtime_error("score_refine_batch_marginals: var_ptr must start at 0");
    sel_ptr.assign(1, 0);
    sel.clear();
    const int dp = U.dp();
    for (int g = 0; g < U.count; ++g) {
        const GbMember& M = U.members[(size_t)g];
        if (var_ptr[g + 1] < var_ptr[g]) throw std::runtime_error("score_refine_batch_marginals: var_ptr must not decrease");
        if (var_ptr[g + 1] > var_ptr[g] && !vars) throw std::runtime_error("score_refine_batch_marginals: vars is null");
        std::vector<char> seen((size_t)(M.Np + M.Nl), 0);
        for (int32_t k = var_ptr[g]; k < var_ptr[g + 1]; ++k) {
            const long long v = vars[k];
            const std::string where = "score_refine_batch_marginals: member " + std::to_string(g) + ": ";
            if (v < 0 || v >= M.Np + M.Nl) throw std::runtime_error(where + "variable out of range");
            if (v == 0) throw std::runtime_error(where + "pose 0 is fixed, it has no covariance");
            if (seen[(size_t)v]) throw std::runtime_error(where + "a variable is listed twice");
            seen[(size_t)v] = 1;
            const long long first = v < M.Np ? (long long)dp * (v - 1) : (long long)dp * (M.Np - 1) + (long long)U.dim * (v - M.Np);
            const int cnt = v < M.Np ? dp : U.dim;
            if ((long long)sel.size() + cnt >= ((long long)1 << 31)) throw std::runtime_error("score_refine_batch_marginals: too many columns");
            for (int q = 0; q < cnt; ++q) sel.push_back((int32_t)(first + q));
        }
        sel_ptr.push_back((int32_t)sel.size());
    }
}

inline int gbm_slots(int most) { return most <= 1 ? 1 : most <= 2 ? 2 : most <= 4 ? 4 : most <= 8 ? 8 : 16; }

// The block's buffers: device allocations of their own (not the handle's arena); they come with the first call, sized for
// the slots it needs, grow on demand and go with the handle.  At 64 worlds of 12 k unknowns a vector is 6 MB: 16 slots x 6
// buffers are about 0.6 GB.
struct GbmWork {
    DevBuf<double> x, r, z, p, w, p_scratch, pw_part, rz0, rz1, rz_prec, ref, res_part, zb;
    DevBuf<int32_t> flags;  // [done: G * NV | steps: G * NV | ... | a zero (the chain kernel's done word) at 2 * G * kMvMaxWidth]
    int slots = 0;
    void reserve(int nv, size_t G, size_t n, size_t n_tiles, size_t n_ublocks, size_t n_prec, size_t zb_per_vector, hipStream_t st) {
        if (nv <= slots) return;
        struct NoArena {
            DevArena* keep;
            NoArena() : keep(tl_arena) { tl_arena = nullptr; }
            ~NoArena() { tl_arena = keep; }
        } no_arena;
        HIP_CHECK(sync_stream(st));  // (nothing queued still reads the buffers that go)
        const size_t wide = (size_t)kMvMaxWidth;
        if (!flags.d) {  // the small ones: for the widest pass at once
            pw_part.alloc(wide * n_tiles); pw_part.zero(st);
            rz0.alloc(wide * n_ublocks); rz0.zero(st);
            rz1.alloc(wide * n_ublocks); rz1.zero(st);
            res_part.alloc(wide * n_ublocks); res_part.zero(st);
            ref.alloc(wide * G); ref.zero(st);
            flags.alloc(2 * wide * G + 1); flags.zero(st);
        }
        DevBuf<double>* vecs[] = {&x, &r, &z, &p, &w, &p_scratch};
        for (DevBuf<double>* v : vecs) { v->alloc((size_t)nv * n); v->zero(st); }
        // (every workgroup of a chain-kernel launch has a slot for its partial of r'z, per vector: written, never read here)
        rz_prec.alloc((size_t)nv * n_prec + 4096); rz_prec.zero(st);
        zb.alloc((size_t)nv * std::max<size_t>(1, zb_per_vector)); zb.zero(st);
        slots = nv;
    }
};

// The solve.  Batch: score_refine_batch (its union, point, blocks and gather, its linear-mode handle, its GbmWork).
template <class Batch>
int gbm_solve(Batch& B, const double* poses, const double* landmarks, const int32_t* var_ptr, const int32_t* vars, double rel_tol,
              int32_t max_iters, int32_t block_width, double* joint, double* residuals, int32_t* iters, score_marginals_batch_info* info) {
    const GbUnion& U = B.U;
    if (block_width < 1 || block_width > kMvMaxWidth) throw std::runtime_error("score_refine_batch_marginals: block_width must be 1..16");
    if (!(rel_tol > 0.0) || max_iters < 1) throw std::runtime_error("score_refine_batch_marginals: rel_tol must be positive and max_iters >= 1");
    std::vector<int32_t> sel_ptr, sel;
    gbm_columns(U, var_ptr, vars, sel_ptr, sel);
    const int G = U.count, n_sel = (int)sel.size(), W = block_width;
    std::vector<long long> joint_off((size_t)G, 0);
    std::vector<int32_t> sel_member((size_t)n_sel, 0);
    size_t joint_size = 0;
    int most_columns = 0;
    for (int g = 0; g < G; ++g) {
        const size_t Cg = (size_t)(sel_ptr[(size_t)g + 1] - sel_ptr[(size_t)g]);
        joint_off[(size_t)g] = (long long)joint_size;
        joint_size += Cg * Cg;
        if (joint_size > ((size_t)1 << 27)) throw std::runtime_error("score_refine_batch_marginals: too many columns for one call (the C_g x C_g doubles beyond 1 GiB)");
        most_columns = std::max(most_columns, (int)Cg);
        std::fill(sel_member.begin() + sel_ptr[(size_t)g], sel_member.begin() + sel_ptr[(size_t)g + 1], g);
    }
    const int passes = (most_columns + W - 1) / W;
    HipBackend& be = B.be();
    hipStream_t st = B.stream();
    const long long n = U.n;
    const double t0 = now_ms();
    // H of every member at its point, on the union pattern, lambda = 0; the chains of all members factored once
    B.set_point(poses, landmarks);
    B.eval(std::vector<char>((size_t)G, 1), false, true, nullptr);
    B.gather_h(std::vector<double>((size_t)G, 0.0).data());
    be.derive_rho_data(false);
    std::vector<int32_t> col_done((size_t)n_sel, 0), col_iters((size_t)n_sel, 0);
    std::vector<double> col_res((size_t)n_sel, 0.0);
    int pcg_iters = 0;
    double t1 = now_ms();
    if (passes > 0) {
        auto& K = B.mvb;
        const size_t zb_per_vector = (size_t)be.H->bs * (size_t)be.n_join_seps;
        K.reserve(gbm_slots(std::min(W, most_columns)), (size_t)G, (size_t)n, (size_t)B.n_tiles, (size_t)B.n_ublocks, (size_t)be.n_prec, zb_per_vector, st);
        DevBuf<int32_t> d_sel_ptr, d_sel, d_sel_member;
        DevBuf<long long> d_joint_off;
        DevBuf<double> d_joint;
        {
            struct NoArena {
                DevArena* keep;
                NoArena() : keep(tl_arena) { tl_arena = nullptr; }
                ~NoArena() { tl_arena = keep; }
            } no_arena;
            d_sel_ptr.alloc((size_t)G + 1); d_sel.alloc((size_t)n_sel); d_sel_member.alloc((size_t)n_sel);
            d_joint_off.alloc((size_t)G); d_joint.alloc(joint_size);
        }
        staged_h2d(d_sel_ptr.d, sel_ptr.data(), ((size_t)G + 1) * sizeof(int32_t), st);
        staged_h2d(d_sel.d, sel.data(), (size_t)n_sel * sizeof(int32_t), st);
        staged_h2d(d_sel_member.d, sel_member.data(), (size_t)n_sel * sizeof(int32_t), st);
        staged_h2d(d_joint_off.d, joint_off.data(), (size_t)G * sizeof(long long), st);
        GbmArgs a{};
        a.d = B.dev();
        a.ptr = be.Kset.mat.ptr.d; a.col = be.Kset.mat.col.d; a.val = be.Kset.mat.val.d;
        a.tiles = B.tiles.d; a.n_tiles = B.n_tiles; a.n_ublocks = B.n_ublocks; a.n = n;
        a.done = K.flags.d; a.ref = K.ref.d;
        a.x = K.x.d; a.r = K.r.d; a.z = K.z.d; a.p = K.p.d; a.w = K.w.d; a.pw_part = K.pw_part.d;
        a.tol2 = rel_tol * rel_tol;
        a.sel_ptr = d_sel_ptr.d; a.sel = d_sel.d; a.sel_member = d_sel_member.d; a.joint_off = d_joint_off.d; a.n_sel = n_sel;
        a.width = W; a.res_part = K.res_part.d; a.joint = d_joint.d;
        int32_t* const zero_word = K.flags.d + 2 * (size_t)kMvMaxWidth * (size_t)G;
        struct ZbScope {  // the chain kernel's second level writes the separators' solutions of the pass's vectors here
            HipBackend& be;
            ZbScope(HipBackend& b, double* zb) : be(b) { be.join_vec_zb = zb; }
            ~ZbScope() { be.join_vec_zb = nullptr; }
        } zb_scope(be, K.zb.d);
        t1 = now_ms();
        const dim3 bt(kThreads), gt((unsigned)B.n_tiles);
        std::vector<int32_t> words;
        std::vector<double> res_part;
        for (int k = 0; k < passes; ++k) {
            int most = 0;
            for (int g = 0; g < G; ++g) most = std::max(most, std::min(W, sel_ptr[(size_t)g + 1] - sel_ptr[(size_t)g] - k * W));
            const int NV = gbm_slots(most);
            a.NV = NV; a.k0 = k * W; a.iters = K.flags.d + (size_t)G * (size_t)NV;
            const dim3 gu((unsigned)B.n_ublocks, (unsigned)NV);
            auto product = [&]() {
                switch (NV) {
                    case 1: hipLaunchKernelGGL(k_gbm_product<1>, gt, bt, 0, st, a); break;
                    case 2: hipLaunchKernelGGL(k_gbm_product<2>, gt, bt, 0, st, a); break;
                    case 4: hipLaunchKernelGGL(k_gbm_product<4>, gt, bt, 0, st, a); break;
                    case 8: hipLaunchKernelGGL(k_gbm_product<8>, gt, bt, 0, st, a); break;
                    default: hipLaunchKernelGGL(k_gbm_product<16>, gt, bt, 0, st, a); break;
                }
            };
            // z = M^-1 r of every slot over the whole group, then the per-workgroup partials of r'z into `rz`
            auto precondition = [&](double* rz) {
                PrecArgs pa = be.prec_args(be.Kset);
                pa.done = zero_word;
                be.prec_vectors(pa, K.r.d, K.r.d, K.z.d, K.p_scratch.d, K.w.d, K.p_scratch.d, K.p_scratch.d, nullptr);
                pa.rz_in = nullptr; pa.rz_out = K.rz_prec.d;
                if (NV > 1) { pa.n_vec = NV; pa.vec_stride = n; }
                be.launch_prec<PREC_INIT>(be.Kset, pa, -1, HipBackend::PrecDepth::join);
                a.rz_part = rz;
                hipLaunchKernelGGL(k_gbm_rz, gu, bt, 0, st, a);
            };
            hipLaunchKernelGGL(k_gbm_rhs, gu, bt, 0, st, a);
            double* rz_cur = K.rz0.d; double* rz_nxt = K.rz1.d;
            precondition(rz_cur);
            a.first = 1; a.rz_new = rz_cur; a.rz_old = nullptr;
            hipLaunchKernelGGL(k_gbm_direction, gu, bt, 0, st, a);
            a.first = 0;
            words.assign(2 * (size_t)G * (size_t)NV, 0);
            int queued = 0;
            bool all_done = false;
            while (!all_done && queued < max_iters) {
                const int chunk = std::min(max_iters - queued, queued == 0 ? 16 : 32);
                for (int j = 0; j < chunk; ++j) {
                    a.all_slots = 0; a.p_in = K.p.d;
                    product();
                    a.rz_new = rz_cur;
                    hipLaunchKernelGGL(k_gbm_step, gu, bt, 0, st, a);
                    precondition(rz_nxt);
                    a.rz_new = rz_nxt; a.rz_old = rz_cur;
                    hipLaunchKernelGGL(k_gbm_direction, gu, bt, 0, st, a);
                    std::swap(rz_cur, rz_nxt);
                }
                queued += chunk;
                HIP_CHECK(hipGetLastError());
                staged_d2h(words.data(), K.flags.d, words.size() * sizeof(int32_t), st);  // (done words and steps: one read)
                all_done = true;
                for (size_t q = 0; q < (size_t)G * (size_t)NV; ++q) all_done = all_done && words[q] != 0;
            }
            // the true residual of every column of the pass (one more product, w = H x), the rows of S
            a.all_slots = 1; a.p_in = K.x.d;
            product();
            hipLaunchKernelGGL(k_gbm_residual, gu, bt, 0, st, a);
            hipLaunchKernelGGL(k_gbm_gather, dim3((unsigned)((n_sel + kThreads - 1) / kThreads), (unsigned)NV), bt, 0, st, a);
            HIP_CHECK(hipGetLastError());
            res_part.resize((size_t)NV * (size_t)B.n_ublocks);
            staged_d2h(res_part.data(), K.res_part.d, res_part.size() * sizeof(double), st);
            int most_steps = 0;
            for (int g = 0; g < G; ++g) {
                const GbMember& M = U.members[(size_t)g];
                const int Cg = sel_ptr[(size_t)g + 1] - sel_ptr[(size_t)g];
                for (int c = 0; c < W && k * W + c < Cg; ++c) {
                    double s = 0.0;  // the member's partials in workgroup order
                    for (int b = M.ublk0; b < M.ublk1; ++b) s += res_part[(size_t)c * (size_t)B.n_ublocks + (size_t)b];
                    const double rho = std::sqrt(s);
                    const size_t at = (size_t)sel_ptr[(size_t)g] + (size_t)(k * W + c), word = (size_t)g * (size_t)NV + (size_t)c;
                    col_res[at] = rho;
                    col_done[at] = (words[word] == 1 && std::isfinite(rho)) ? 1 : 0;
                    col_iters[at] = words[(size_t)G * (size_t)NV + word];
                    most_steps = std::max(most_steps, col_iters[at]);
                }
            }
            pcg_iters += most_steps;
        }
        if (joint && joint_size) staged_d2h(joint, d_joint.d, joint_size * sizeof(double), st);
        HIP_CHECK(sync_stream(st));
    }
    const double t2 = now_ms();
    int unconverged = 0;
    double worst = 0.0;
    for (int c = 0; c < n_sel; ++c) {
        if (!col_done[(size_t)c]) ++unconverged;
        worst = std::isfinite(col_res[(size_t)c]) ? std::max(worst, col_res[(size_t)c]) : INFINITY;
        if (residuals) residuals[c] = col_res[(size_t)c];
        if (iters) iters[c] = col_done[(size_t)c] ? col_iters[(size_t)c] : -(col_iters[(size_t)c] + 1);
    }
    if (info) {
        info->columns = n_sel; info->passes = passes; info->pcg_iters = pcg_iters; info->unconverged = unconverged;
        info->max_residual = worst; info->setup_ms = t1 - t0; info->solve_ms = t2 - t1;
    }
    return unconverged ? 1 : 0;
}

}  // namespace score

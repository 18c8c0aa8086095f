// score_group_pcg.hpp -- the gated conjugate-gradient iteration of a refinement group, stated once: every (member, slot) pair
// of a union problem (score_gn_batch.hpp) has its own alpha, beta, gate and done word.  Two callers:
//   the lock-step Levenberg-Marquardt step (score_refine_batch::solve): ONE slot, the right-hand side -g of every live member
//   (k_gb_pcg_begin); the members a round leaves out start with done word 1
//   the marginals of a group (score_marginals_batch.hpp): NV = 1, 2, 4, 8 or 16 slots, one unit column of every member per slot
//   (k_gbm_rhs)
//
// H = J'J of the union is block diagonal, so ONE union vector carries one right-hand side of EVERY member: the NV vectors of a
// pass are stored one after the other with stride U.n (the layout PrecArgs::vec_stride expects) and advance in one pass over the
// union matrix.  Per-slot words: done[g NV + c], iters[g NV + c], ref[g NV + c].  Partials: pw_part[c n_tiles + tile],
// rz_part[c n_ublocks + workgroup].  Every workgroup of the kernels below belongs to one member -- taken from tiles[].w or
// ublk_member[] --, tests the done word of its (member, slot) first, and leaves a done slot's x, r and p as they are.  One
// iteration:
//   k_gbm_product    w_c = H p_c for the live slots of the tile's member from ONE pass over the union CSR (64 short rows x 4
//                    lanes, or one long row over the workgroup: mv_product_tile of score_marginals.hpp), per-tile partials of p'w
//   k_gbm_step       alpha = r'z / p'w of (member, slot), both re-reduced in fixed order over the member's own partial ranges
//                    [tile0, tile1) and [ublk0, ublk1) at the slot's offset; x += alpha p, r -= alpha w
//   M^-1             z_c = M^-1 r_c, every slot of the whole group in one launch of the chain kernel
//                    (HipBackend::precondition_block; a done slot's z is scratch)
//   k_gbm_rz         per-workgroup partials of r_c'z_c: a kernel of its own, so that no item straddles members
//   k_gbm_direction  beta = r'z_new / r'z_old, p = z + beta p; the gate r'z_new <= rel_tol^2 r0'z0 raises the slot's done word
// The decisions of k_gbm_step and k_gbm_direction are pcg_step_rule and pcg_direction_rule of score_marginals.hpp, the ones
// k_mv_step and k_mv_direction take; the re-reduction over the member's own ranges and the word layout are this file's.
// Done words: 1 converged (or nothing to solve), 2 broken down (a non-finite r'z or p'w, or p'w <= 0) -- reported as failure.
// No atomics: all workgroups of a (member, slot) reduce the same partials in the same order and take the same decision.
#pragma once

#include <cstdint>
#include <vector>

#include "score_gn_batch.hpp"
#include "score_marginals.hpp"

namespace score {

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
    // the columns of the marginals (zero in the Levenberg-Marquardt solve): member g selects the member-local unknowns
    // sel[sel_ptr[g] .. sel_ptr[g + 1])
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

// grid (unknown workgroups): x = 0, r = rhs on the members about to be solved (done word 0) -- the one slot of the
// Levenberg-Marquardt solve, whose words the host has set
__global__ __launch_bounds__(kThreads) void k_gb_pcg_begin(GbmArgs a, const double* __restrict__ rhs) {
    const int g = a.d.ublk_member[blockIdx.x];
    if (a.done[g]) return;
    const GbMember M = a.d.members[g];
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + threadIdx.x;
    if (li < M.n) {
        a.x[M.col0 + li] = 0.0;
        a.r[M.col0 + li] = rhs[M.col0 + li];
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

inline void gbm_product(const GbmArgs& a, hipStream_t st) {
    mv_with_slots(a.NV, [&](auto nv) {
        hipLaunchKernelGGL(k_gbm_product<decltype(nv)::value>, dim3((unsigned)a.n_tiles), dim3(kThreads), 0, st, a);
    });
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
    double alpha;
    if (!pcg_step_rule(rz, pw, alpha)) {
        if (lead) a.done[word] = kPcgBroken;
        return;
    }
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
    double beta;
    const int verdict = pcg_direction_rule(a.first != 0, rzn, rzo, a.ref + word, beta);
    if (verdict == kPcgConverged || verdict == kPcgBroken) {
        if (lead) a.done[word] = verdict;
        return;
    }
    if (verdict == kPcgThreshold && lead) a.ref[word] = a.tol2 * rzn;
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + t;
    if (li < M.n) {
        const long long e = c * a.n + M.col0 + li;
        a.p[e] = a.first ? a.z[e] : a.z[e] + beta * a.p[e];
    }
}

// The iteration's buffers, all zeroed when they come, from the arena in scope (none: device allocations of their own).  The
// small ones are sized once, for `width` slots; the vectors hold `slots` and grow on demand -- the caller has made sure that
// nothing queued still reads the ones that go.
struct GroupPcgWork {
    DevBuf<double> x, r, z, p, w, scratch, pw_part, rz0, rz1, rz_prec, ref;
    DevBuf<int32_t> flags;  // [done: G * NV | steps: G * NV | ... | a zero (the chain kernel's done word) at 2 * G * width]
    size_t G = 0;
    int width = 0, slots = 0;
    int32_t* zero_word() const { return flags.d + 2 * G * (size_t)width; }
    void reserve(int nv, int widest, size_t members, size_t n, size_t n_tiles, size_t n_ublocks, size_t n_prec, hipStream_t st) {
        if (!flags.d) {
            G = members; width = widest;
            const size_t wide = (size_t)widest;
            pw_part.alloc(wide * n_tiles); pw_part.zero(st);
            rz0.alloc(wide * n_ublocks); rz0.zero(st);
            rz1.alloc(wide * n_ublocks); rz1.zero(st);
            ref.alloc(wide * G); ref.zero(st);
            flags.alloc(2 * wide * G + 1); flags.zero(st);
        }
        if (nv <= slots) return;
        DevBuf<double>* vecs[] = {&x, &r, &z, &p, &w, &scratch};
        for (DevBuf<double>* v : vecs) { v->alloc((size_t)nv * n); v->zero(st); }
        // (every workgroup of a chain-kernel launch has a slot for its partial of r'z, per vector: written, never read here)
        rz_prec.alloc((size_t)nv * n_prec + 4096); rz_prec.zero(st);
        slots = nv;
    }
};

// The iteration of NV slots, queued on the backend's stream.  `a`: the union, its matrix and tiles, tol2 and whatever the
// caller's own kernels read; the words, vectors and partials of K are set here, and `a` is left ready for a product of the
// caller's (the residual's).  rhs(a): the launch that sets x = 0 and r of every live slot (and the words, where the host has
// not).  zb: the separators' solutions of the NV vectors in the chain kernel's second level (null for one slot).  `words`:
// the done words then the step counts, [g * NV + c] each, as they stand after the last chunk queued.
template <class Rhs>
inline void group_pcg(HipBackend& be, GbmArgs& a, GroupPcgWork& K, int NV, int max_iters, double* zb, Rhs rhs, std::vector<int32_t>& words) {
    hipStream_t st = be.stream;
    const size_t slots = K.G * (size_t)NV;
    a.NV = NV; a.done = K.flags.d; a.iters = K.flags.d + slots; a.ref = K.ref.d;
    a.x = K.x.d; a.r = K.r.d; a.z = K.z.d; a.p = K.p.d; a.w = K.w.d; a.pw_part = K.pw_part.d;
    a.all_slots = 0; a.p_in = K.p.d;
    const dim3 bt(kThreads), gu((unsigned)a.n_ublocks, (unsigned)NV);
    // z = M^-1 r of every slot over the whole group, then the per-workgroup partials of r'z into `rz`
    auto precondition = [&](double* rz) {
        be.precondition_block(K.r.d, K.z.d, K.scratch.d, K.w.d, NV, a.n, K.zero_word(), K.rz_prec.d, zb);
        a.rz_part = rz;
        hipLaunchKernelGGL(k_gbm_rz, gu, bt, 0, st, a);
    };
    rhs(a);
    double* rz_cur = K.rz0.d; double* rz_nxt = K.rz1.d;
    precondition(rz_cur);
    a.first = 1; a.rz_new = rz_cur; a.rz_old = nullptr;
    hipLaunchKernelGGL(k_gbm_direction, gu, bt, 0, st, a);
    a.first = 0;
    words.assign(2 * slots, 0);
    queue_in_chunks(max_iters, [&]() {
        gbm_product(a, st);
        a.rz_new = rz_cur;
        hipLaunchKernelGGL(k_gbm_step, gu, bt, 0, st, a);
        precondition(rz_nxt);
        a.rz_new = rz_nxt; a.rz_old = rz_cur;
        hipLaunchKernelGGL(k_gbm_direction, gu, bt, 0, st, a);
        std::swap(rz_cur, rz_nxt);
    }, [&]() {
        staged_d2h(words.data(), K.flags.d, words.size() * sizeof(int32_t), st);  // (done words and steps: one read)
        return std::all_of(words.begin(), words.begin() + (std::ptrdiff_t)slots, [](int32_t f) { return f != 0; });
    });
}

}  // namespace score

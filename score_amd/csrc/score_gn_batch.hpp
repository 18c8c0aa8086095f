// score_gn_batch.hpp -- local refinement of a GROUP of graphs in lock-step (include/score_refine_batch.h).
//
// One union problem: member g owns the unknowns [col0_g, col0_g + n_g), H = J'J is block diagonal, and ONE linear-mode handle
// on the union pattern -- its chain hint lists every member's chains -- gives derive_rho_data / k_factor / launch_prec<PREC_INIT>
// for the whole group unchanged (M^-1 is block diagonal: chains and Jacobi columns never span members).  Per-member control:
// every workgroup of every kernel here belongs to exactly one member (work is padded at member boundaries), tests that
// member's mask or done word first, and writes nothing for a member that is masked out or done.
//
// The state holds every pose, pins included: 2-D [theta, x, y] per pose then the landmarks, 3-D [R | t] per pose then the
// landmarks, member after member -- the single handle's layout.  A workgroup builds its member's GnView (gb_view) and calls the
// lane functions of score_gn.hpp that the single handle's kernels call, and a member's measurements are laid over workgroups
// exactly as k_gn_blocks lays them (local measurement m in the member's workgroup m / kThreads), so a member's cost partials
// are those of a handle on it alone.
//
// The damped step of a round is one slot of the group's conjugate-gradient iteration (score_group_pcg.hpp, shared with the
// marginals of a group): every member has its own alpha, beta, gate and done word, and a member the round leaves out starts
// with done word 1.  The product's tiles of a member are cut by mv_tiles (score_marginals.hpp) from its own rows.
//
// The controller is gb_lock_step (score_refine_drivers.hpp): one LmState per member, the step rule of score_refine_rule.hpp.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "../../include/score_refine_batch.h"
#include "score_gn.hpp"
#include "score_kernels.hpp"
#include "score_marginals.hpp"

namespace score {

// ---------------------------------------------------------------------------
// the union problem
// ---------------------------------------------------------------------------
struct GbMember {  // where member g lives in the union arrays
    long long Np, Nl, n, n_rel, n_rng, n_pri;
    long long rel0, rng0, pri0;        // first entry in the measurement arrays
    long long state0, col0;            // first scalar of its state, its first unknown
    long long hblk0, gblk0;            // first slot of its block storage
    long long pose0, lm0;              // first scalar in the caller's pose / landmark arrays
    int mblk0, mblk1, ublk0, ublk1, sblk0, sblk1, tile0, tile1;  // its workgroups: measurements, unknowns, variables, product tiles
    // the robust refinement (score_gn_robust_batch.hpp): its loop closures are the trailing n_lc relative-pose entries, lc0 is
    // the first of them in the group's loop-closure order; its workgroups over ranges + loop closures
    long long n_lc, lc0;
    int rblk0, rblk1;
};

struct GbUnion : GnMeas {  // (the measurement arrays: the members' one after the other)
    int dim = 2, count = 0;
    long long n = 0, state_size = 0, hblk_size = 0, gblk_size = 0, poses_size = 0, lms_size = 0, lcs_size = 0;
    std::vector<char> lc_short;  // [member] fewer relative-pose entries than odometry steps: its loop closures cannot be re-weighted
    std::vector<GbMember> members;
    std::vector<int32_t> hptr, hcol, hc_ptr, hc_slot, gc_ptr, gc_slot, diag_member;  // diag_member[k]: member + 1 on a diagonal entry, else 0
    std::vector<int32_t> chain_ptr, node_first_col;
    std::vector<int32_t> mblk_member, ublk_member, sblk_member, rblk_member;
    std::vector<int4> tiles;  // {first row, end row, long row?, member}
    int dp() const { return dim == 2 ? 3 : 6; }
    int pose_scalars() const { return dim == 2 ? 3 : 12; }
};

// gn_build member by member, the members' patterns and contribution lists laid one after the other with offsets
inline void gb_build(const score_graph* graphs, int count, GbUnion& U) {
    if (count <= 0 || !graphs) throw std::runtime_error("score_refine_batch: no graphs");
    U = GbUnion{};
    U.dim = graphs[0].dim;
    U.count = count;
    U.hptr.assign(1, 0); U.hc_ptr.assign(1, 0); U.gc_ptr.assign(1, 0); U.chain_ptr.assign(1, 0);
    const long long lim = (long long)1 << 31;
    for (int g = 0; g < count; ++g) {
        if (graphs[g].dim != U.dim) throw std::runtime_error("score_refine_batch: the graphs of a group must share dim");
        GnProblem P;
        gn_build(graphs[g], P);
        if (P.n <= 0) throw std::runtime_error("score_refine_batch: a member has no unknowns");
        GbMember M{};
        M.Np = P.Np; M.Nl = P.Nl; M.n = P.n; M.n_rel = P.n_rel(); M.n_rng = P.n_rng(); M.n_pri = P.n_pri();
        M.rel0 = U.n_rel(); M.rng0 = U.n_rng(); M.pri0 = U.n_pri();
        M.state0 = U.state_size; M.col0 = U.n; M.hblk0 = U.hblk_size; M.gblk0 = U.gblk_size;
        M.pose0 = U.poses_size; M.lm0 = U.lms_size;
        long long odometry = 0;
        for (int32_t len : P.chain_len) odometry += (long long)len - 1;
        M.n_lc = std::max<long long>(0, M.n_rel - odometry); M.lc0 = U.lcs_size;
        U.lc_short.push_back(M.n_rel < odometry ? 1 : 0);
        const long long nnz0 = (long long)U.hcol.size(), hs0 = (long long)U.hc_slot.size(), gs0 = (long long)U.gc_slot.size();
        if (M.col0 + P.n >= lim / 64 || nnz0 + (long long)P.hcol.size() >= lim || hs0 + (long long)P.hc_slot.size() >= lim ||
            M.hblk0 + P.hblk_size() >= lim || M.state0 + (long long)U.pose_scalars() * P.Np + U.dim * P.Nl >= lim ||
            M.rel0 + M.n_rel >= lim || M.rng0 + M.n_rng >= lim || M.lc0 + M.n_lc >= lim ||
            4 * ((long long)U.rblk_member.size() + (M.n_rng + M.n_lc) / kThreads + 1) >= lim)
            throw std::runtime_error("score_refine_batch: the group is too large for 32-bit positions (use smaller groups)");
        U.append(P);
        for (long long i = 0; i < P.n; ++i) {
            U.hptr.push_back((int32_t)(nnz0 + P.hptr[(size_t)i + 1]));
            U.gc_ptr.push_back((int32_t)(gs0 + P.gc_ptr[(size_t)i + 1]));
        }
        for (size_t k = 0; k < P.hcol.size(); ++k) {
            U.hcol.push_back((int32_t)(M.col0 + P.hcol[k]));
            U.hc_ptr.push_back((int32_t)(hs0 + P.hc_ptr[k + 1]));
        }
        U.diag_member.resize(U.hcol.size(), 0);
        for (long long i = 0; i < P.n; ++i) U.diag_member[(size_t)(nnz0 + P.diag_pos[(size_t)i])] = g + 1;
        for (int32_t s : P.hc_slot) U.hc_slot.push_back((int32_t)(M.hblk0 + s));
        for (int32_t s : P.gc_slot) U.gc_slot.push_back((int32_t)(M.gblk0 + s));
        const int32_t node0 = U.chain_ptr.back();
        for (size_t c = 1; c < P.chain_ptr.size(); ++c) U.chain_ptr.push_back(node0 + P.chain_ptr[c]);
        for (int32_t c : P.node_first_col) U.node_first_col.push_back((int32_t)(M.col0 + c));
        // workgroups: measurements, unknowns, variables -- kThreads each, never across a member boundary
        auto blocks = [](long long items) { return (int)std::max<long long>(1, (items + kThreads - 1) / kThreads); };
        M.mblk0 = (int)U.mblk_member.size(); U.mblk_member.insert(U.mblk_member.end(), (size_t)blocks(P.n_meas()), g); M.mblk1 = (int)U.mblk_member.size();
        M.ublk0 = (int)U.ublk_member.size(); U.ublk_member.insert(U.ublk_member.end(), (size_t)blocks(P.n), g); M.ublk1 = (int)U.ublk_member.size();
        M.sblk0 = (int)U.sblk_member.size(); U.sblk_member.insert(U.sblk_member.end(), (size_t)blocks(P.Np + P.Nl), g); M.sblk1 = (int)U.sblk_member.size();
        M.rblk0 = (int)U.rblk_member.size(); U.rblk_member.insert(U.rblk_member.end(), (size_t)blocks(M.n_rng + M.n_lc), g); M.rblk1 = (int)U.rblk_member.size();
        // product tiles of the member's rows
        M.tile0 = (int)U.tiles.size();
        mv_tiles(P.hptr, P.n, U.tiles, M.col0, g);
        M.tile1 = (int)U.tiles.size();
        U.n += P.n;
        U.state_size += (long long)U.pose_scalars() * P.Np + (long long)U.dim * P.Nl;
        U.hblk_size += P.hblk_size(); U.gblk_size += P.gblk_size();
        U.poses_size += (long long)U.pose_scalars() * P.Np; U.lms_size += (long long)U.dim * P.Nl; U.lcs_size += M.n_lc;
        U.members.push_back(M);
    }
}

// ---------------------------------------------------------------------------
// device side
// ---------------------------------------------------------------------------
struct GbDev {
    const GbMember* members;
    const int32_t *mblk_member, *ublk_member, *sblk_member, *rblk_member;
    GnMeasPtr meas;  // the union's measurement arrays
};

// member M of the group as a lane sees it (GnView, score_gn.hpp): the union arrays from its first entry (gn_meas_from, which
// the host can call too: tests/tools/refine_view_check.cpp), its state in X, its block storage in hblk / gblk (null: none)
template <int DIM>
__device__ __forceinline__ GnView gb_view(const GbDev& d, const GbMember& M, const double* X, double* hblk, double* gblk) {
    GnView v;
    v.Np = M.Np; v.Nl = M.Nl; v.n_rel = M.n_rel; v.n_rng = M.n_rng; v.n_pri = M.n_pri;
    v.meas = gn_meas_from<DIM>(d.meas, M.rel0, M.rng0, M.pri0);
    v.X = X + M.state0;
    v.hblk = hblk ? hblk + M.hblk0 : nullptr; v.gblk = gblk ? gblk + M.gblk0 : nullptr;
    return v;
}

// one measurement per lane (gn_measurement on the member's view): cost partial of the workgroup and, with_blocks, its
// J'J / J'r block
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gb_blocks(GbDev d, const double* __restrict__ X, double* __restrict__ hblk,
                                                        double* __restrict__ gblk, double* __restrict__ cost_part,
                                                        const int32_t* __restrict__ mask, int with_blocks) {
    __shared__ double red[8];
    const int g = d.mblk_member[blockIdx.x];
    if (!mask[g]) return;
    const GbMember M = d.members[g];
    const long long m = (long long)((int)blockIdx.x - M.mblk0) * kThreads + threadIdx.x;
    const double tot = block_sum(gn_measurement<DIM>(gb_view<DIM>(d, M, X, hblk, gblk), m, with_blocks != 0), red);
    if (threadIdx.x == 0) cost_part[blockIdx.x] = tot;
}

// one variable (pose or landmark) per lane: dst = retract(src, step) on the masked members (gn_retract_variable).
// step == nullptr: the copy of `accept` (dst = X, src = Xt).  The pinned pose of a member has no step.
template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gb_trial(GbDev d, const double* __restrict__ src, const double* __restrict__ step,
                                                       double* __restrict__ dst, const int32_t* __restrict__ mask) {
    const int g = d.sblk_member[blockIdx.x];
    if (!mask[g]) return;
    const GbMember M = d.members[g];
    const long long i = (long long)((int)blockIdx.x - M.sblk0) * kThreads + threadIdx.x;
    gn_retract_variable<DIM>(src + M.state0, step ? step + M.col0 : nullptr, dst + M.state0, M.Np, M.Nl, i);
}

// one entry of H per lane: the sum of its block slots in list order (+ the member's lambda on the diagonal)
__global__ __launch_bounds__(kThreads) void k_gb_gather_h(const int32_t* __restrict__ hc_ptr, const int32_t* __restrict__ hc_slot,
                                                          const double* __restrict__ hblk, const int32_t* __restrict__ diag_member,
                                                          const double* __restrict__ lambda, double* __restrict__ out, long long nnz) {
    const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (k >= nnz) return;
    double acc = 0.0;
    for (int32_t c = hc_ptr[k]; c < hc_ptr[k + 1]; ++c) acc += hblk[hc_slot[c]];
    const int dm = diag_member[k];
    out[k] = dm ? acc + lambda[dm - 1] : acc;
}

// one unknown per lane, on the masked members: g = J'r, rhs = -g, workgroup partial of |g|_inf
__global__ __launch_bounds__(kThreads) void k_gb_gather_g(GbDev d, const int32_t* __restrict__ gc_ptr, const int32_t* __restrict__ gc_slot,
                                                          const double* __restrict__ gblk, double* __restrict__ rhs,
                                                          double* __restrict__ gmax_part, const int32_t* __restrict__ mask) {
    __shared__ double red[8];
    const int g = d.ublk_member[blockIdx.x];
    if (!mask[g]) return;
    const GbMember M = d.members[g];
    const long long li = (long long)((int)blockIdx.x - M.ublk0) * kThreads + threadIdx.x;
    double a = 0.0;
    if (li < M.n) {
        const long long i = M.col0 + li;
        double acc = 0.0;
        for (int32_t c = gc_ptr[i]; c < gc_ptr[i + 1]; ++c) acc += gblk[gc_slot[c]];
        rhs[i] = -acc;
        a = acc == acc ? fabs(acc) : INFINITY;
    }
    const double mx = block_max(a, red);
    if (threadIdx.x == 0) gmax_part[blockIdx.x] = mx;
}

}  // namespace score

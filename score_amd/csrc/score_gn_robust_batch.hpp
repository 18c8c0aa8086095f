// score_gn_robust_batch.hpp -- outlier-robust refinement of a GROUP of graphs in lock-step (include/score_refine_robust_batch.h):
// the GNC-TLS outer loop of score_gn_robust.hpp, one per member, around the lock-step Levenberg-Marquardt rounds of
// score_gn_batch.hpp on one group handle.
//
// Device: the two kernels of score_gn_robust.hpp over the union problem, around the same lane functions.  One measurement per
// lane, a member's ranges first and then its loop closures (its trailing n_lc relative-pose entries), padded at member
// boundaries (rblk_member, rblk0 / rblk1 of GbMember); a workgroup tests its member's mask word first and writes nothing for a
// member that is masked out.
//   k_gbr_resid    gn_robust_resid_lane on the member's view (gb_view): r at the member's point in the union state, with the
//                  MEASURED precisions (prec0, kappa0, tau0: arrays of the handle's own, the loop closures in loop-closure order);
//                  per workgroup and family max r^2 (non-finite r: +inf) and the count of non-binary weights.  The host folds a
//                  member's partials in workgroup order (gn_robust_fold), as a handle on the member alone does.
//   k_gbr_weight   reads the member's GbrParam: gn_robust_weight in the member's enabled families -- w = gnc_tls_weight(r, mu, c_f)
//                  (mu = 0: w = 1) -- and by `mode` the precisions k_gb_blocks reads (rng_prec, rel_kappa, rel_tau).
// Host: gbr_lock_step (score_refine_drivers.hpp), gb_lock_step plus a GncState per member: the schedule of score_refine_rule.hpp,
// as gn_robust_refine drives it on one handle.
#pragma once

#include "../../include/score_refine_robust_batch.h"
#include "score_gn_batch.hpp"
#include "score_gn_robust.hpp"

namespace score {

struct GbrDev {
    GbDev d;
    GnRobustArrays a;         // the union's: ranges as rng_*, loop closures in loop-closure order
    const GbrParam* params;   // [member]
};

template <int DIM>
__global__ __launch_bounds__(kThreads) void k_gbr_resid(GbrDev a, const double* __restrict__ X, double* __restrict__ part,
                                                        const int32_t* __restrict__ mask) {
    __shared__ double red[8];
    const GbDev& d = a.d;
    const int g = d.rblk_member[blockIdx.x];
    if (!mask[g]) return;
    const GbMember M = d.members[g];
    const long long i = (long long)((int)blockIdx.x - M.rblk0) * kThreads + threadIdx.x;
    gn_robust_resid_lane<DIM>(gb_view<DIM>(d, M, X, nullptr, nullptr), a.a, i, M.n_rng, M.n_lc, M.rng0 + i, M.lc0 + (i - M.n_rng),
                              M.n_rel - M.n_lc, red, part + (long long)kGnRobustPart * blockIdx.x);
}

__global__ __launch_bounds__(kThreads) void k_gbr_weight(GbrDev d, const int32_t* __restrict__ mask) {
#pragma clang fp contract(off)
    const GnRobustArrays& a = d.a;
    const int g = d.d.rblk_member[blockIdx.x];
    if (!mask[g]) return;
    const GbMember M = d.d.members[g];
    const GbrParam p = d.params[g];
    const long long i = (long long)((int)blockIdx.x - M.rblk0) * kThreads + threadIdx.x;
    const bool from_r = p.mode == kGbrNext || p.mode == kGbrInspect;   // then: in the enabled families only
    if (i < M.n_rng) {
        if (from_r && !(p.families & kGnRobustRanges)) return;
        const long long e = M.rng0 + i;
        const double f = gn_robust_weight(p.mode, a.r_rng + e, a.w_rng + e, p.mu, p.c_rng, p.min_weight);
        if (p.mode != kGbrInspect) a.prec[e] = a.prec0[e] * f;
    } else if (i < M.n_rng + M.n_lc) {
        if (from_r && !(p.families & kGnRobustClosures)) return;
        const long long q = i - M.n_rng, e = M.lc0 + q, m = M.rel0 + (M.n_rel - M.n_lc) + q;
        const double f = gn_robust_weight(p.mode, a.r_lc + e, a.w_lc + e, p.mu, p.c_lc, p.min_weight);
        if (p.mode != kGbrInspect) { a.kappa[m] = a.kappa0[e] * f; a.tau[m] = a.tau0[e] * f; }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// gn_robust_check on member g's measured precisions (prec: its ranges; kappa, tau: its loop closures)
inline void gbr_check(const score_refine_robust_settings& s, int g, const double* prec, long long n_rng, const double* kappa,
                      const double* tau, long long n_lc) {
    gn_robust_check_settings("score_refine_batch_robust_run: member " + std::to_string(g) + ": ", s, prec, n_rng, kappa, tau, n_lc);
}

}  // namespace score

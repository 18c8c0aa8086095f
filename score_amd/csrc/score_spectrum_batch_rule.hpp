// score_spectrum_batch_rule.hpp -- the rule that moves one member of a group through the block eigensolver
// (include/score_spectrum_batch.h), stated once and free of HIP: a state record with its transitions as pure functions, in
// the style of score_refine_rule.hpp.  It is sp_solve's loop (score_spectrum.hpp) cut where the group's driver reads the
// device: once per lock-step round, after the residual norms of every live member stand.
//
// A round of the driver (gsp_solve, score_spectrum_batch.hpp):
//   first half   verifying members: AX = A X, the true product.  Iterating and verifying members: R = AX - theta X, the
//                16 norms, the done words
//   the read     the norms and the status of the last Rayleigh-Ritz step, O(count) words; gsp_after_residual per live member
//   second half  iterating members: W = M^-1 R, AW = A W, the Gram pass, Rayleigh-Ritz, combine
// so a member that the rule sends back from verifying to iterating takes its second half in the same round: its residual
// block and done words are those of the true product, which is what sp_solve recomputes at the top of its loop.
//
// The rule, as there: the first k columns done by the recurrence's AX -> look again with the product (verify); done by the
// product too -> finished; not done -> go on iterating, AX exact again.  A member whose iteration count reaches max_iters, or
// whose Rayleigh-Ritz step broke down, gets one last verification and ends on its verdict: it ends only on the residuals of
// a true product.  A finished or broken member is no longer touched.
#pragma once

#include <cstdint>

namespace score {

enum GspMode : int32_t { kGspIterate = 0, kGspVerify = 1, kGspFinished = 2, kGspBroken = 3 };
constexpr int kGspRitzBreakdown = 2;  // (= kSpRrBreakdown of score_spectrum_rr.hpp, asserted where both are seen)

struct GspState {
    GspMode mode = kGspIterate;
    int32_t iterations = 0;       // Rayleigh-Ritz steps taken on [X | W | P] (the start block's orthonormalisation is none)
    bool started = false;         // the start block's Rayleigh-Ritz step has been seen
    bool ritz_pending = true;     // the member's last second half (or the start) ran a Rayleigh-Ritz step not yet seen
    bool has_p = false;           // P holds directions
    bool last = false;            // the verification under way ends the member whatever it finds
    bool broke = false;
    bool converged = false;       // finished with all k pairs at tolerance, by the product
};

inline bool gsp_live(const GspState& s) { return s.mode == kGspIterate || s.mode == kGspVerify; }

// the control word of the member as the kernels read it
inline int32_t gsp_word(const GspState& s) { return (int32_t)s.mode | (s.has_p ? 1 << 8 : 0); }

// (a non-finite norm is not done)
inline bool gsp_first_k_done(const double* norms, int k, double tol) {
    for (int c = 0; c < k; ++c)
        if (!(norms[c] <= tol)) return false;
    return true;
}

inline void gsp_begin(GspState& s) { s = GspState{}; }

// The read of a round: `norms` are the member's 16 residual norms of the first half, ritz_status the status of its last
// Rayleigh-Ritz step (read only where one is pending).  Afterwards: kGspIterate -- the second half runs for the member;
// kGspVerify -- the next first half forms its product; kGspFinished / kGspBroken -- its X, values and norms stand.
inline void gsp_after_residual(GspState& s, const double* norms, int k, double tol, int ritz_status, int max_iters) {
    if (s.mode == kGspIterate) {
        if (s.ritz_pending) {
            s.ritz_pending = false;
            if (ritz_status == kGspRitzBreakdown) {  // (X and its values are as they were before the step)
                s.broke = s.last = true;
                s.mode = kGspVerify;
                return;
            }
            if (s.started) { s.iterations += 1; s.has_p = true; }
            s.started = true;
        }
        if (s.iterations >= max_iters) { s.last = true; s.mode = kGspVerify; return; }
        if (gsp_first_k_done(norms, k, tol)) { s.mode = kGspVerify; return; }
        s.ritz_pending = true;
        return;
    }
    if (s.mode != kGspVerify) return;
    if (s.broke) { s.mode = kGspBroken; return; }
    if (gsp_first_k_done(norms, k, tol)) { s.converged = true; s.mode = kGspFinished; return; }
    if (s.last) { s.mode = kGspFinished; return; }
    s.mode = kGspIterate;  // AX is exact again; this round's second half has columns to work on
    s.ritz_pending = true;
}

// what the call reports for the member: its iterations, as -(it + 1) where not all k pairs converged or it broke down
inline int32_t gsp_reported_iterations(const GspState& s) { return s.converged ? s.iterations : -(s.iterations + 1); }

}  // namespace score

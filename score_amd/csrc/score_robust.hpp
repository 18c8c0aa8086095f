// score_robust.hpp -- the device half of score_robust_solve_rel (include/score_robust.h): GNC-TLS re-weighting of the range
// measurements and of the loop closures between outer solves.
//
// After every outer solve, over all ranges of the handle's problems (one thread per range):
//   k_robust_resid   r = sqrt(prec) max(0, |t_a - t_b| - dist) from the solution on the device (x = xhat * D, the
//                    translations k_read_estimates reads); per problem: max r^2, and how many weights of this solve are
//                    more than 1e-6 from 0 and from 1
//   k_robust_weight  the problem's mu (mu0 = c^2 / (2 max r^2 - c^2) after the first solve, mu_step * mu after later ones),
//                    the GNC-TLS weight, the next precision prec max(w, min_weight) -- into the members' home arrays and into
//                    the compact array the next handle is built from; per problem: largest weight change, inliers
//   k_robust_gather  when members stop: the measurement arrays of the members still running, compacted in their order
// The loop closures (the trailing relative-pose entries of every problem) are the second family, one thread per loop closure:
//   k_robust_resid_rel   r = sqrt(kappa |t_j - t_i - R_i t~|^2 + tau |R_j - R_i R~|_F^2) from the relaxed blocks [R | t] of the
//                        solution (the pinned pose is [I | 0]), the measured kappa and tau; the same per-problem reductions
//                        into the family's own control records
//   k_robust_weight_rel  the weight and the next kappa, tau -- home and compact, as for the ranges
// Both residual kernels run before either weight kernel: a problem's first mu is the smallest of the enabled families'
// c_f^2 / (2 max r_f^2 - c_f^2) (robust_mu: every weight kernel computes it from both families' control records).
// The per-problem reductions are max and integer sums only (a wave reduces first where all 64 lanes hold one problem, one
// atomic per lane otherwise): the control records do not depend on the order the waves run in.
#pragma once
#include <hip/hip_runtime.h>

#include "score_assemble.hpp"
#include "score_setup_device.hpp"

namespace score {

struct RobustCtl {               // one per member and family (home order): what the host reads after every outer solve
    unsigned long long r2max;    // bits of the largest r^2 (non-negative doubles order as their bit patterns)
    unsigned long long dwmax;    // bits of the largest |w_next - w|
    int32_t inliers;             // measurements with w_next >= 1/2
    int32_t nonbinary;           // measurements whose weight in this solve is more than 1e-6 from both 0 and 1
};

struct RobustArgs {
    int32_t d, count;                 // the handle's problems = the members still running, in handle order
    int32_t first;                    // 1: the members' first solve
    const EstProb* probs;             // count: the handle's layout (score_assemble.hpp)
    const int32_t* rng_off;           // count + 1: first range of each problem in the handle
    const int32_t* member;            // count: the member (home index) of each problem
    const int32_t* home_rng_off;      // members + 1
    int64_t n_rng;                    // ranges of the handle
    const double* x; const double* D; // the equilibrated solution and its column scales
    const int32_t* rng_a; const int32_t* rng_b; const double* rng_dist;   // compact (handle order)
    const double* prec;               // home: the measured precisions
    const double* w;                  // home: weights of this solve
    double* resid;                    // home: r
    double* w_next; double* prec_next;   // home
    double* prec_work;                // compact: rng_prec of the next handle (same members)
    RobustCtl* ctl;                   // home
    const RobustCtl* ctl_other;       // home: the loop closures' records (null: that family is off)
    const double* mu_in; double* mu_out;  // home
    double c, c_other, mu_step, min_weight;
};

// the weight rule (the host twin is score_amd/robust.py: gnc_tls_weight -- same operations, same order)
__device__ __forceinline__ double gnc_tls_weight(double r, double mu, double c) {
#pragma clang fp contract(off)
    const double r2 = r * r, c2 = c * c;
    if (r2 <= mu / (mu + 1.0) * c2) return 1.0;
    if (r2 >= (mu + 1.0) / mu * c2) return 0.0;
    return c / r * sqrt(mu * (mu + 1.0)) - mu;
}

// mu0 of one family after the first solve: c^2 / (2 max r^2 - c^2), 0 where the family has no outlier (2 max r^2 <= c^2)
__device__ __forceinline__ double robust_mu0(const RobustCtl& R, double c) {
#pragma clang fp contract(off)
    const double c2 = c * c;
    const double r2max = __longlong_as_double((long long)R.r2max);
    return 2.0 * r2max <= c2 ? 0.0 : c2 / (2.0 * r2max - c2);
}
// the problem's mu for the weights that follow this solve: after the first solve the smallest mu0 of the families with
// outliers (0: none has any, every weight stays 1), mu_step * mu after later ones
__device__ __forceinline__ double robust_mu(int first, const RobustCtl& own, double c, const RobustCtl* other, double c_other,
                                            double mu_in, double mu_step) {
#pragma clang fp contract(off)
    if (!first) return mu_in * mu_step;
    double mu = robust_mu0(own, c);
    if (other) {
        const double mo = robust_mu0(*other, c_other);
        if (mo > 0.0 && (mu == 0.0 || mo < mu)) mu = mo;
    }
    return mu;
}

// per-problem max / sum of one value per lane: a wave whose live lanes all hold problem m0 reduces first (lane 0 does the
// atomics); otherwise every live lane does its own
__device__ __forceinline__ void robust_reduce(bool live, int m, double vmax, int32_t cnt, RobustCtl* ctl, bool second) {
    const int m0 = __shfl(m, 0);
    const bool uniform = __all(!live || m == m0);
    if (uniform) {
        double v = live ? vmax : 0.0;
        int32_t c = live ? cnt : 0;
        for (int o = 32; o > 0; o >>= 1) {
            v = fmax(v, __shfl_xor(v, o));
            c += __shfl_xor(c, o);
        }
        if (threadIdx.x % 64 == 0 && m0 >= 0) {
            RobustCtl& R = ctl[m0];
            atomicMax(second ? &R.dwmax : &R.r2max, (unsigned long long)__double_as_longlong(v));
            if (c) atomicAdd(second ? &R.inliers : &R.nonbinary, c);
        }
    } else if (live) {
        RobustCtl& R = ctl[m];
        atomicMax(second ? &R.dwmax : &R.r2max, (unsigned long long)__double_as_longlong(vmax));
        if (cnt) atomicAdd(second ? &R.inliers : &R.nonbinary, cnt);
    }
}

struct RobustRange { int p, m; int64_t home; };
__device__ __forceinline__ RobustRange robust_range(const RobustArgs& a, int64_t i) {
    RobustRange q;
    q.p = a.count > 1 ? tab_find(a.rng_off, a.count, i) : 0;
    q.m = a.member[q.p];
    q.home = (int64_t)a.home_rng_off[q.m] + (i - a.rng_off[q.p]);
    return q;
}

__global__ __launch_bounds__(256) void k_robust_resid(RobustArgs a) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < a.n_rng;
    int m = -1;
    double r2 = 0.0;
    int32_t nonbin = 0;
    if (live) {
        const RobustRange q = robust_range(a, i);
        m = q.m;
        const EstProb P = a.probs[q.p];
        const int d = a.d, D1 = d + 1;
        const int64_t lm0 = (int64_t)(P.Np - 1) * D1;
        auto xv = [&](int64_t local) { const int64_t c = P.xoff + local; return a.x[c] * a.D[c]; };
        auto tvar = [&](int64_t v, int k) {
            if (v < P.Np) return v == 0 ? 0.0 : xv((int64_t)k * P.n_rep + (v - 1) * D1 + d);
            return xv((int64_t)k * P.n_rep + lm0 + (v - P.Np));
        };
        const int64_t va = a.rng_a[i], vb = a.rng_b[i];
        double nn = 0.0;
        for (int k = 0; k < d; ++k) {
            const double dl = tvar(va, k) - tvar(vb, k);
            nn += dl * dl;
        }
        const double r = sqrt(a.prec[q.home]) * fmax(0.0, sqrt(nn) - a.rng_dist[i]);
        a.resid[q.home] = r;
        r2 = r * r;
        const double wi = a.w[q.home];
        nonbin = (fabs(wi) <= 1e-6 || fabs(1.0 - wi) <= 1e-6) ? 0 : 1;
    }
    robust_reduce(live, m, r2, nonbin, a.ctl, false);
}

__global__ __launch_bounds__(256) void k_robust_weight(RobustArgs a) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < a.n_rng;
    int m = -1;
    double dw = 0.0;
    int32_t inl = 0;
    if (live) {
        const RobustRange q = robust_range(a, i);
        m = q.m;
        // (a first solve without outliers keeps w = 1: mu = 0 marks it)
        const double mu = robust_mu(a.first, a.ctl[m], a.c, a.ctl_other ? a.ctl_other + m : nullptr, a.c_other, a.mu_in[m], a.mu_step);
        const double wn = mu > 0.0 ? gnc_tls_weight(a.resid[q.home], mu, a.c) : 1.0;
        const double pn = a.prec[q.home] * fmax(wn, a.min_weight);
        a.w_next[q.home] = wn;
        a.prec_next[q.home] = pn;
        a.prec_work[i] = pn;
        if (i == a.rng_off[q.p]) a.mu_out[m] = mu;
        dw = fabs(wn - a.w[q.home]);
        inl = wn >= 0.5 ? 1 : 0;
    }
    robust_reduce(live, m, dw, inl, a.ctl, true);
}

// ---- the loop closures: the trailing n_lc relative-pose entries of every problem ----
struct RobustRelArgs {
    int32_t d, count;                 // as RobustArgs
    int32_t first;
    const EstProb* probs;
    const int32_t* lc_off;            // count + 1: first loop closure of each problem among the handle's loop closures
    const int32_t* rel_off;           // count + 1: first relative-pose entry of each problem in the handle (compact arrays)
    const int32_t* member;            // count
    const int32_t* home_lc_off;       // members + 1
    const int32_t* home_rel_off;      // members + 1
    int64_t n_lc;                     // loop closures of the handle
    const double* x; const double* D;
    const int32_t* rel_base; const int32_t* rel_to; const double* rel_t; const double* rel_R;   // compact (handle order)
    const double* kappa; const double* tau;   // home relative-pose arrays: the measured precisions
    const double* w;                  // home (loop-closure order): weights of this solve
    double* resid;                    // home: r
    double* w_next; double* kappa_next; double* tau_next;   // home
    double* kappa_work; double* tau_work;   // compact relative-pose arrays: rel_kappa / rel_tau of the next handle
    RobustCtl* ctl;                   // home: the loop closures' records
    const RobustCtl* ctl_other;       // home: the ranges' records (null: that family is off)
    const double* mu_in; double* mu_out;
    double c, c_other, mu_step, min_weight;
};

struct RobustLc { int p, m; int64_t home, rel, home_rel; };   // home: among the members' loop closures; rel: entry of the arrays
__device__ __forceinline__ RobustLc robust_lc(const RobustRelArgs& a, int64_t i) {
    RobustLc q;
    q.p = a.count > 1 ? tab_find(a.lc_off, a.count, i) : 0;
    q.m = a.member[q.p];
    const int64_t local = i - a.lc_off[q.p], n_lc = (int64_t)a.lc_off[q.p + 1] - a.lc_off[q.p];
    q.home = (int64_t)a.home_lc_off[q.m] + local;
    q.rel = (int64_t)a.rel_off[q.p + 1] - n_lc + local;
    q.home_rel = (int64_t)a.home_rel_off[q.m + 1] - n_lc + local;
    return q;
}

__global__ __launch_bounds__(256) void k_robust_resid_rel(RobustRelArgs a) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < a.n_lc;
    int m = -1;
    double r2 = 0.0;
    int32_t nonbin = 0;
    if (live) {
        const RobustLc q = robust_lc(a, i);
        m = q.m;
        const EstProb P = a.probs[q.p];
        const int d = a.d, D1 = d + 1;
        auto xv = [&](int64_t local) { const int64_t c = P.xoff + local; return a.x[c] * a.D[c]; };
        // entry (k, c) of the relaxed block [R | t] of pose v; the pinned pose is [I | 0]
        auto blk = [&](int64_t v, int k, int c) {
            if (v == 0) return k == c ? 1.0 : 0.0;
            return xv((int64_t)k * P.n_rep + (v - 1) * D1 + c);
        };
        const int64_t vi = a.rel_base[q.rel], vj = a.rel_to[q.rel];
        const double* tm = a.rel_t + q.rel * d;
        const double* Rm = a.rel_R + q.rel * d * d;
        double st = 0.0, sR = 0.0;
        for (int k = 0; k < d; ++k) {
            double Ri[3];
            for (int c = 0; c < d; ++c) Ri[c] = blk(vi, k, c);
            double s = 0.0;
            for (int c = 0; c < d; ++c) s += Ri[c] * tm[c];
            const double dl = blk(vj, k, d) - blk(vi, k, d) - s;
            st += dl * dl;
            for (int c = 0; c < d; ++c) {
                double u = 0.0;
                for (int j = 0; j < d; ++j) u += Ri[j] * Rm[j * d + c];
                const double dr = blk(vj, k, c) - u;
                sR += dr * dr;
            }
        }
        const double r = sqrt(a.kappa[q.home_rel] * st + a.tau[q.home_rel] * sR);
        a.resid[q.home] = r;
        r2 = r * r;
        const double wi = a.w[q.home];
        nonbin = (fabs(wi) <= 1e-6 || fabs(1.0 - wi) <= 1e-6) ? 0 : 1;
    }
    robust_reduce(live, m, r2, nonbin, a.ctl, false);
}

__global__ __launch_bounds__(256) void k_robust_weight_rel(RobustRelArgs a) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < a.n_lc;
    int m = -1;
    double dw = 0.0;
    int32_t inl = 0;
    if (live) {
        const RobustLc q = robust_lc(a, i);
        m = q.m;
        const double mu = robust_mu(a.first, a.ctl[m], a.c, a.ctl_other ? a.ctl_other + m : nullptr, a.c_other, a.mu_in[m], a.mu_step);
        const double wn = mu > 0.0 ? gnc_tls_weight(a.resid[q.home], mu, a.c) : 1.0;
        const double f = fmax(wn, a.min_weight);
        const double kn = a.kappa[q.home_rel] * f, tn = a.tau[q.home_rel] * f;
        a.w_next[q.home] = wn;
        a.kappa_next[q.home] = kn; a.tau_next[q.home] = tn;
        a.kappa_work[q.rel] = kn; a.tau_work[q.rel] = tn;
        if (i == a.lc_off[q.p]) a.mu_out[m] = mu;   // (the range kernel writes the same value)
        dw = fabs(wn - a.w[q.home]);
        inl = wn >= 0.5 ? 1 : 0;
    }
    robust_reduce(live, m, dw, inl, a.ctl, true);
}

struct RobustGatherArgs {
    int32_t d, count, with_static;    // with_static = 0: the precisions only
    const int32_t* member;            // count
    const int32_t* rel_off; const int32_t* rng_off;            // count + 1: compact offsets
    const int32_t* home_rel_off; const int32_t* home_rng_off;  // members + 1
    int64_t n_rel, n_rng;             // compact totals
    const int32_t* h_rel_base; const int32_t* h_rel_to; const double* h_rel_t; const double* h_rel_R;
    const double* h_rel_kappa; const double* h_rel_tau;
    const int32_t* home_lc_off;       // members + 1, with the two arrays below (null: the loop closures keep their measured precisions)
    const double* h_kappa_next; const double* h_tau_next;   // home (loop-closure order): the weighted kappa, tau
    const int32_t* h_rng_a; const int32_t* h_rng_b; const double* h_rng_dist; const double* h_prec;
    int32_t* rel_base; int32_t* rel_to; double* rel_t; double* rel_R; double* rel_kappa; double* rel_tau;
    int32_t* rng_a; int32_t* rng_b; double* rng_dist; double* prec;
};
__global__ __launch_bounds__(256) void k_robust_gather(RobustGatherArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int d = a.d;
    if (a.with_static && i < a.n_rel) {
        const int p = a.count > 1 ? tab_find(a.rel_off, a.count, i) : 0;
        const int64_t h = (int64_t)a.home_rel_off[a.member[p]] + (i - a.rel_off[p]);
        a.rel_base[i] = a.h_rel_base[h]; a.rel_to[i] = a.h_rel_to[h];
        for (int k = 0; k < d; ++k) a.rel_t[i * d + k] = a.h_rel_t[h * d + k];
        for (int k = 0; k < d * d; ++k) a.rel_R[i * d * d + k] = a.h_rel_R[h * d * d + k];
        a.rel_kappa[i] = a.h_rel_kappa[h]; a.rel_tau[i] = a.h_rel_tau[h];
        if (a.h_kappa_next) {  // a loop closure: the precisions the last weight kernel wrote
            const int m = a.member[p];
            const int64_t n_lc = (int64_t)a.home_lc_off[m + 1] - a.home_lc_off[m];
            const int64_t lc = (i - a.rel_off[p]) - ((int64_t)(a.rel_off[p + 1] - a.rel_off[p]) - n_lc);
            if (lc >= 0) { a.rel_kappa[i] = a.h_kappa_next[a.home_lc_off[m] + lc]; a.rel_tau[i] = a.h_tau_next[a.home_lc_off[m] + lc]; }
        }
    }
    if (i < a.n_rng) {
        const int p = a.count > 1 ? tab_find(a.rng_off, a.count, i) : 0;
        const int64_t h = (int64_t)a.home_rng_off[a.member[p]] + (i - a.rng_off[p]);
        a.prec[i] = a.h_prec[h];
        if (a.with_static) { a.rng_a[i] = a.h_rng_a[h]; a.rng_b[i] = a.h_rng_b[h]; a.rng_dist[i] = a.h_rng_dist[h]; }
    }
}

}  // namespace score

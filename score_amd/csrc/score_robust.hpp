// score_robust.hpp -- the device half of score_robust_solve_rel (include/score_robust.h, the host half is score_robust_driver.hpp):
// GNC-TLS re-weighting of the range measurements and of the loop closures between outer solves.
//
// A re-weighted FAMILY of measurements is stated once: a record of its arrays with three methods (locate, residual, apply), and
// the two kernel templates run any family, one thread per item of the handle's problems:
//   k_robust_resid<Family>   r = Family::residual from the solution on the device (x = xhat * D, what k_read_estimates reads);
//                            per problem: max r^2, and how many weights of this solve are more than 1e-6 from 0 and from 1
//   k_robust_weight<Family>  the problem's mu (robust_mu: after the first solve the smallest c_f^2 / (2 max r_f^2 - c_f^2) of the
//                            enabled families, from both families' control records; mu_step * mu after later ones), the GNC-TLS
//                            weight w, Family::apply(max(w, min_weight)) -- the next precisions into the members' home arrays and
//                            into the compact arrays the next handle is built from; per problem: largest weight change, inliers
// The families:
//   RobustRanges    r = sqrt(prec) max(0, |t_a - t_b| - dist) on the solution's translations; apply scales prec
//   RobustClosures  the loop closures, the trailing relative-pose entries of every problem:
//                   r = sqrt(kappa |t_j - t_i - R_i t~|^2 + tau |R_j - R_i R~|_F^2) on the relaxed blocks [R | t] (the pinned pose
//                   is [I | 0]) with the measured kappa, tau; apply scales both
// Both families' residual kernels run before either weight kernel: the first mu needs both maxima.
//   k_robust_gather  when members stop: the measurement arrays of the members still running, compacted in their order
// The per-problem reductions are max and integer sums only (a wave reduces first where all 64 lanes hold one problem, one
// atomic per lane otherwise): the control records do not depend on the order the waves run in.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "score_assemble.hpp"
#include "score_refine_rule.hpp"   // RobustSeen, robust_decide: the stop rule of the host loops
#include "score_setup_device.hpp"

namespace score {

struct RobustCtl {               // one per member and family (home order): what the host reads after every outer solve
    unsigned long long r2max;    // bits of the largest r^2 (non-negative doubles order as their bit patterns)
    unsigned long long dwmax;    // bits of the largest |w_next - w|
    int32_t inliers;             // measurements with w_next >= 1/2
    int32_t nonbinary;           // measurements whose weight in this solve is more than 1e-6 from both 0 and 1
};

struct RobustShared {             // what every family's kernels read
    int32_t d, count, first;          // count: the handle's problems = the members still running, in handle order; first = 1: their first solve
    const EstProb* probs;             // count: the handle's layout (score_assemble.hpp)
    const int32_t* member;            // count: the member (home index) of each problem
    const double* x; const double* D; // the equilibrated solution and its column scales
    const double* mu_in; double* mu_out;  // home
    double mu_step, min_weight;
};

struct RobustFamily {             // what the kernels need of any family
    const int32_t* off;               // count + 1: first item of each problem among the handle's items of this family
    const int32_t* home_off;          // members + 1
    int64_t n;                        // items of the handle
    const double* w; double* resid; double* w_next;   // home: weights of this solve, r, weights of the next
    RobustCtl* ctl; const RobustCtl* ctl_other;       // home: its records, the other family's (null: that family is off)
    double c, c_other;
};

template <class Family> struct RobustArgs { RobustShared s; Family f; };

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

// where item i of a family (or entry i of a compact array) lives: its problem, its member, its home index; `at` / `home_at`:
// its entry in the compact / home measurement arrays (the loop closures sit at the tail of the relative-pose arrays)
struct RobustItem { int p, m; int64_t home, at, home_at; };
__device__ __forceinline__ RobustItem robust_locate(const int32_t* off, const int32_t* home_off, const int32_t* member, int count, int64_t i) {
    RobustItem q;
    q.p = count > 1 ? tab_find(off, count, i) : 0;
    q.m = member[q.p];
    q.home = (int64_t)home_off[q.m] + (i - off[q.p]);
    q.at = i; q.home_at = q.home;
    return q;
}

struct RobustRanges : RobustFamily {
    const int32_t* a; const int32_t* b; const double* dist;   // compact (handle order)
    const double* prec; double* prec_next;   // home: the measured precisions, those of the next solve
    double* prec_work;                // compact: rng_prec of the next handle (same members)

    __device__ __forceinline__ RobustItem locate(const RobustShared& s, int64_t i) const { return robust_locate(off, home_off, s.member, s.count, i); }
    __device__ __forceinline__ double residual(const RobustShared& s, const RobustItem& q) const {
#pragma clang fp contract(off)
        const EstProb P = s.probs[q.p];
        const int d = s.d, D1 = d + 1;
        const int64_t lm0 = (int64_t)(P.Np - 1) * D1;
        auto xv = [&](int64_t local) { const int64_t c = P.xoff + local; return s.x[c] * s.D[c]; };
        auto tvar = [&](int64_t v, int k) {
            if (v < P.Np) return v == 0 ? 0.0 : xv((int64_t)k * P.n_rep + (v - 1) * D1 + d);
            return xv((int64_t)k * P.n_rep + lm0 + (v - P.Np));
        };
        const int64_t va = a[q.at], vb = b[q.at];
        double nn = 0.0;
        for (int k = 0; k < d; ++k) {
            const double dl = tvar(va, k) - tvar(vb, k);
            nn += dl * dl;
        }
        return sqrt(prec[q.home_at]) * fmax(0.0, sqrt(nn) - dist[q.at]);
    }
    __device__ __forceinline__ void apply(const RobustItem& q, double f) const {
#pragma clang fp contract(off)
        const double pn = prec[q.home_at] * f;
        prec_next[q.home] = pn; prec_work[q.at] = pn;
    }
};

struct RobustClosures : RobustFamily {
    const int32_t* rel_off;           // count + 1: first relative-pose entry of each problem in the handle (compact arrays)
    const int32_t* home_rel_off;      // members + 1
    const int32_t* rel_base; const int32_t* rel_to; const double* rel_t; const double* rel_R;   // compact (handle order)
    const double* kappa; const double* tau;   // home relative-pose arrays: the measured precisions
    double* kappa_next; double* tau_next;     // home (loop-closure order)
    double* kappa_work; double* tau_work;     // compact relative-pose arrays: rel_kappa / rel_tau of the next handle

    __device__ __forceinline__ RobustItem locate(const RobustShared& s, int64_t i) const {
        RobustItem q = robust_locate(off, home_off, s.member, s.count, i);
        const int64_t local = i - off[q.p], n_lc = (int64_t)off[q.p + 1] - off[q.p];
        q.at = (int64_t)rel_off[q.p + 1] - n_lc + local;
        q.home_at = (int64_t)home_rel_off[q.m + 1] - n_lc + local;
        return q;
    }
    __device__ __forceinline__ double residual(const RobustShared& s, const RobustItem& q) const {
#pragma clang fp contract(off)
        const EstProb P = s.probs[q.p];
        const int d = s.d, D1 = d + 1;
        auto xv = [&](int64_t local) { const int64_t c = P.xoff + local; return s.x[c] * s.D[c]; };
        // entry (k, c) of the relaxed block [R | t] of pose v; the pinned pose is [I | 0]
        auto blk = [&](int64_t v, int k, int c) {
            if (v == 0) return k == c ? 1.0 : 0.0;
            return xv((int64_t)k * P.n_rep + (v - 1) * D1 + c);
        };
        const int64_t vi = rel_base[q.at], vj = rel_to[q.at];
        const double* tm = rel_t + q.at * d;
        const double* Rm = rel_R + q.at * d * d;
        double st = 0.0, sR = 0.0;
        for (int k = 0; k < d; ++k) {
            double Ri[3];
            for (int c = 0; c < d; ++c) Ri[c] = blk(vi, k, c);
            double sm = 0.0;
            for (int c = 0; c < d; ++c) sm += Ri[c] * tm[c];
            const double dl = blk(vj, k, d) - blk(vi, k, d) - sm;
            st += dl * dl;
            for (int c = 0; c < d; ++c) {
                double u = 0.0;
                for (int j = 0; j < d; ++j) u += Ri[j] * Rm[j * d + c];
                const double dr = blk(vj, k, c) - u;
                sR += dr * dr;
            }
        }
        return sqrt(kappa[q.home_at] * st + tau[q.home_at] * sR);
    }
    __device__ __forceinline__ void apply(const RobustItem& q, double f) const {
#pragma clang fp contract(off)
        const double kn = kappa[q.home_at] * f, tn = tau[q.home_at] * f;
        kappa_next[q.home] = kn; tau_next[q.home] = tn;
        kappa_work[q.at] = kn; tau_work[q.at] = tn;
    }
};

template <class Family>
__global__ __launch_bounds__(256) void k_robust_resid(RobustArgs<Family> a) {
#pragma clang fp contract(off)
    const RobustShared& s = a.s; const Family& F = a.f;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < F.n;
    int m = -1; double r2 = 0.0; int32_t nonbin = 0;
    if (live) {
        const RobustItem q = F.locate(s, i); m = q.m;
        const double r = F.residual(s, q);
        F.resid[q.home] = r;
        r2 = r * r;
        const double wi = F.w[q.home];
        nonbin = (fabs(wi) <= 1e-6 || fabs(1.0 - wi) <= 1e-6) ? 0 : 1;
    }
    robust_reduce(live, m, r2, nonbin, F.ctl, false);
}

template <class Family>
__global__ __launch_bounds__(256) void k_robust_weight(RobustArgs<Family> a) {
#pragma clang fp contract(off)
    const RobustShared& s = a.s; const Family& F = a.f;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < F.n;
    int m = -1; double dw = 0.0; int32_t inl = 0;
    if (live) {
        const RobustItem q = F.locate(s, i); m = q.m;
        // (a first solve without outliers keeps w = 1: mu = 0 marks it)
        const double mu = robust_mu(s.first, F.ctl[m], F.c, F.ctl_other ? F.ctl_other + m : nullptr, F.c_other, s.mu_in[m], s.mu_step);
        const double wn = mu > 0.0 ? gnc_tls_weight(F.resid[q.home], mu, F.c) : 1.0;
        F.w_next[q.home] = wn;
        F.apply(q, fmax(wn, s.min_weight));
        if (i == F.off[q.p]) s.mu_out[m] = mu;   // (every family's first item writes the same value)
        dw = fabs(wn - F.w[q.home]);
        inl = wn >= 0.5 ? 1 : 0;
    }
    robust_reduce(live, m, dw, inl, F.ctl, true);
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
        const RobustItem q = robust_locate(a.rel_off, a.home_rel_off, a.member, a.count, i);
        const int p = q.p, m = q.m; const int64_t h = q.home;
        a.rel_base[i] = a.h_rel_base[h]; a.rel_to[i] = a.h_rel_to[h];
        for (int k = 0; k < d; ++k) a.rel_t[i * d + k] = a.h_rel_t[h * d + k];
        for (int k = 0; k < d * d; ++k) a.rel_R[i * d * d + k] = a.h_rel_R[h * d * d + k];
        a.rel_kappa[i] = a.h_rel_kappa[h]; a.rel_tau[i] = a.h_rel_tau[h];
        if (a.h_kappa_next) {  // a loop closure: the precisions the last weight kernel wrote
            const int64_t n_lc = (int64_t)a.home_lc_off[m + 1] - a.home_lc_off[m];
            const int64_t lc = (i - a.rel_off[p]) - ((int64_t)(a.rel_off[p + 1] - a.rel_off[p]) - n_lc);
            if (lc >= 0) { a.rel_kappa[i] = a.h_kappa_next[a.home_lc_off[m] + lc]; a.rel_tau[i] = a.h_tau_next[a.home_lc_off[m] + lc]; }
        }
    }
    if (i < a.n_rng) {
        const int64_t h = robust_locate(a.rng_off, a.home_rng_off, a.member, a.count, i).home;
        a.prec[i] = a.h_prec[h];
        if (a.with_static) { a.rng_a[i] = a.h_rng_a[h]; a.rng_b[i] = a.h_rng_b[h]; a.rng_dist[i] = a.h_rng_dist[h]; }
    }
}

}  // namespace score

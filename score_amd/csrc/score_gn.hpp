// score_gn.hpp -- local refinement after SCORE: Gauss-Newton with
// Levenberg-Marquardt damping on SE(d)^N x R^(d L), d = 2 or 3 (the reference's model is dimension-generic,
// gurobi_utils.py:37-50), shared by the HIP backend and the CPU twin.
//
// 3-D: the state holds every pose as [R (3 x 3, row-major) | t]; a step lives in the tangent space,
// (omega, v) per pose with the retraction R <- R Exp(omega), t <- t + v, so the unknowns of pose p are the six
// columns 6 (p - 1) .. +5 = [omega | v].  The preconditioner's chains are 3 x 3 as in 2-D: per robot one chain
// over the omega blocks and one over the v blocks (their strong couplings run pose to pose within the same
// kind; the omega-v cross blocks are left to the PCG: 84 against 32 iterations with exact 6 x 6 chain blocks
// on a 4 x 300-pose graph -- and no 6 x 6 variant of the chain kernels to carry).
//
// The reference's README (README.md:63-67) hands the SCORE estimate to a local nonlinear least-squares
// solver (GTSAM) for the maximum-likelihood estimate; this is that step over exactly the factors SCORE
// reads (relative poses with the chordal rotation cost gurobi_utils.py:504-526, ranges :449-501,
// landmark priors :433-446):
//
//   F = sum_rel  kappa |t_j - t_i - R(th_i) t_ij|^2 + tau |R(th_j) - R(th_i) R_ij|_F^2
//     + sum_rng  w (|p_a - p_b| - d)^2  +  sum_prior  w |l - l0|^2
//
// Unknowns u = [th_p, x_p, y_p for poses p = 1.. | landmarks (x, y)]; pose 0 (first pose of chain 0) is
// held where SCORE put it.  The state holds every pose, pose 0 included ([theta, x, y] per pose, then the
// landmarks; 3-D below): pose 0 has no unknowns, so it never receives a step.  Per measurement a small dense
// block J_e'J_e and gradient J_e'r_e is computed (one lane / loop iteration each: `gn_measurement` over
// `gn_rel_block`, `gn_range_block`, `gn_prior_block`, compiled for both sides and for the single handle and
// the group alike), every entry of H = J'J and g = J'r then sums its contributions in a fixed order
// (contribution lists built once on the host) -- no atomics, same sums on both backends.  The damped
// normal equations go through the handle's linear mode (score_linear_solve's core: k_factor on the pose
// chains, k_prec_pre + k_spmv PCG).  The LM loop (`gn_lm_run`, score_refine_drivers.hpp) drives the step rule of score_refine_rule.hpp as
// score_amd/refine.py::_lm_loop drives its Python twin, which the tests run beside it with SciPy's sparse LU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "../../include/score_hip.h"
#include "score_host.hpp"
#include "score_refine_drivers.hpp"

#if defined(__HIPCC__)
#define SCORE_GN_HD __host__ __device__ __forceinline__
#else
#define SCORE_GN_HD inline
#endif

namespace score {

// point of a range endpoint (variable id: pose or landmark) in the 2-D state: [theta, x, y] of every pose, then the landmarks
SCORE_GN_HD const double* gn_point2(const double* X, int64_t Np, int64_t v) {
    return v < Np ? X + 3 * v + 1 : X + 3 * Np + 2 * (v - Np);
}

// What a measurement's block is made of, stated once per kind: gn_*_jac gives the whitened residual r and, with_jac, the
// Jacobian J of r in the measurement's local unknowns (rows in the order of r[]); gn_*_block forms the cost r'r and the
// products J'J and J'r of it (gn_normal_products), the posterior samples (score_samples.hpp) form J'z for their own z
// (gn_jt_vec).
template <int N>
SCORE_GN_HD void gn_normal_products(const double (*J)[N], const double* r, double* H, double* g) {  // H = J'J (row-major), g = J'r
    for (int a = 0; a < N; ++a) {
        double ga = 0.0;
        for (int k = 0; k < N; ++k) ga += J[k][a] * r[k];
        g[a] = ga;
        for (int b = 0; b < N; ++b) {
            double h = 0.0;
            for (int k = 0; k < N; ++k) h += J[k][a] * J[k][b];
            H[a * N + b] = h;
        }
    }
}
template <int N>
SCORE_GN_HD void gn_jt_vec(const double (*J)[N], const double* z, double* out) {  // out = J'z, summed over the rows in ascending order
#pragma unroll
    for (int a = 0; a < N; ++a) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) s += J[k][a] * z[k];
        out[a] = s;
    }
}

// relative-pose measurement i -> j.  Local unknowns [th_i, x_i, y_i, th_j, x_j, y_j].  r (6): sqrt(kappa) (t_j - t_i - R_i tm),
// then sqrt(tau) (R_j - R_i Rm) row-major; with_jac: J = dr/d(local unknowns), 6 x 6.
SCORE_GN_HD void gn_rel_jac(double thi, double xi, double yi, double thj, double xj, double yj, const double* tm,
                            const double* Rm, double kappa, double tau, double* r, double (*J)[6], bool with_jac) {
    const double sk = sqrt(kappa), st = sqrt(tau);
    const double ci = cos(thi), si = sin(thi), cj = cos(thj), sj = sin(thj);
    r[0] = sk * (xj - xi - (ci * tm[0] - si * tm[1]));
    r[1] = sk * (yj - yi - (si * tm[0] + ci * tm[1]));
    // R_j - R_i Rm, row-major
    r[2] = st * (cj - (ci * Rm[0] - si * Rm[2]));
    r[3] = st * (-sj - (ci * Rm[1] - si * Rm[3]));
    r[4] = st * (sj - (si * Rm[0] + ci * Rm[2]));
    r[5] = st * (cj - (si * Rm[1] + ci * Rm[3]));
    if (!with_jac) return;
    for (int a = 0; a < 6; ++a)
        for (int b = 0; b < 6; ++b) J[a][b] = 0.0;
    // d(R_i tm)/dth_i
    const double dRt0 = -si * tm[0] - ci * tm[1], dRt1 = ci * tm[0] - si * tm[1];
    J[0][0] = -sk * dRt0; J[0][1] = -sk; J[0][4] = sk;
    J[1][0] = -sk * dRt1; J[1][2] = -sk; J[1][5] = sk;
    // -(dR_i Rm), dR_i = [[-s, -c], [c, -s]]
    J[2][0] = -st * (-si * Rm[0] - ci * Rm[2]);
    J[3][0] = -st * (-si * Rm[1] - ci * Rm[3]);
    J[4][0] = -st * (ci * Rm[0] - si * Rm[2]);
    J[5][0] = -st * (ci * Rm[1] - si * Rm[3]);
    J[2][3] = st * -sj; J[3][3] = st * -cj; J[4][3] = st * cj; J[5][3] = st * -sj;
}
// The curvature term of the measurement, sum_q r_q grad^2 r_q, added to its 6 x 6 block H: d^2 R / d theta^2 = -R, and r is
// additively separable in i and j, so only (th_i, th_i) and (th_j, th_j) get a term.  r: what gn_rel_jac gave at the point.
SCORE_GN_HD void gn_rel_curv(double thi, double thj, const double* tm, const double* Rm, double kappa, double tau, const double* r,
                             double* H) {
    const double sk = sqrt(kappa), st = sqrt(tau);
    const double ci = cos(thi), si = sin(thi), cj = cos(thj), sj = sin(thj);
    // d^2 r / d th_i^2 = + sqrt(kappa) R_i tm (rows 0, 1), + sqrt(tau) R_i Rm (rows 2..5); d^2 r / d th_j^2 = - sqrt(tau) R_j
    const double hi = sk * (r[0] * (ci * tm[0] - si * tm[1]) + r[1] * (si * tm[0] + ci * tm[1]))
                    + st * (r[2] * (ci * Rm[0] - si * Rm[2]) + r[3] * (ci * Rm[1] - si * Rm[3])
                          + r[4] * (si * Rm[0] + ci * Rm[2]) + r[5] * (si * Rm[1] + ci * Rm[3]));
    const double hj = -st * (r[2] * cj - r[3] * sj + r[4] * sj + r[5] * cj);
    H[0] += hi;
    H[3 * 6 + 3] += hj;
}
// Returns the cost r'r; with H / g non-null also J'J (6 x 6, row-major) and J'r (6); exact: H is J'J plus the curvature term.
SCORE_GN_HD double gn_rel_block(double thi, double xi, double yi, double thj, double xj, double yj, const double* tm,
                                const double* Rm, double kappa, double tau, double* H, double* g, bool exact = false) {
    double r[6], J[6][6];
    gn_rel_jac(thi, xi, yi, thj, xj, yj, tm, Rm, kappa, tau, r, J, H != nullptr);
    double cost = 0.0;
    for (int k = 0; k < 6; ++k) cost += r[k] * r[k];
    if (!H) return cost;
    gn_normal_products<6>(J, r, H, g);
    if (exact) gn_rel_curv(thi, thj, tm, Rm, kappa, tau, r, H);
    return cost;
}

// range measurement between points a and b.  Local unknowns [xa, ya, xb, yb].  Returns r = sqrt(prec) (|a - b| - dist); J
// (with_jac): its one row (4).
SCORE_GN_HD double gn_range_jac(double xa, double ya, double xb, double yb, double dist, double prec, double* J, bool with_jac) {
    const double sw = sqrt(prec);
    const double dx = xa - xb, dy = ya - yb;
    const double rho = sqrt(dx * dx + dy * dy);
    const double r = sw * (rho - dist);
    if (with_jac) {
        const bool tiny = !(rho > 1e-12);
        const double g0 = tiny ? 0.0 : dx / rho, g1 = tiny ? 0.0 : dy / rho;
        J[0] = sw * g0; J[1] = sw * g1; J[2] = -sw * g0; J[3] = -sw * g1;
    }
    return r;
}
// The curvature term of a range in D dimensions, r grad^2 r = r sqrt(prec) (I - u u') / rho with u = (a - b) / rho, added to the
// 2 D x 2 D block H: on (a, a) and (b, b), with the opposite sign on (a, b) and (b, a); nothing where rho <= 1e-12, as the
// Jacobian.  d = a - b.
template <int D>
SCORE_GN_HD void gn_range_curv(const double* d, double prec, double r, double* H) {
    double rho2 = 0.0;
    for (int k = 0; k < D; ++k) rho2 += d[k] * d[k];
    const double rho = sqrt(rho2);
    if (!(rho > 1e-12)) return;
    const double s = r * sqrt(prec) / rho;
    for (int a = 0; a < D; ++a)
        for (int b = 0; b < D; ++b) {
            const double t = s * ((a == b ? 1.0 : 0.0) - (d[a] / rho) * (d[b] / rho));
            H[a * 2 * D + b] += t;
            H[(D + a) * 2 * D + D + b] += t;
            H[a * 2 * D + D + b] -= t;
            H[(D + a) * 2 * D + b] -= t;
        }
}
// the cost r'r; with H / g: H 4 x 4, g 4; exact: H with the curvature term.
SCORE_GN_HD double gn_range_block(double xa, double ya, double xb, double yb, double dist, double prec, double* H, double* g,
                                  bool exact = false) {
    double J[4];
    const double r = gn_range_jac(xa, ya, xb, yb, dist, prec, J, H != nullptr);
    if (H) {
        for (int a = 0; a < 4; ++a) {
            g[a] = J[a] * r;
            for (int b = 0; b < 4; ++b) H[a * 4 + b] = J[a] * J[b];
        }
        if (exact) {
            const double d[2] = {xa - xb, ya - yb};
            gn_range_curv<2>(d, prec, r, H);
        }
    }
    return r * r;
}

// landmark prior.  Local unknowns [lx, ly].  r (2) = sqrt(prec) (l - t0); returns the Jacobian: sqrt(prec) times the identity.
SCORE_GN_HD double gn_prior_jac(double lx, double ly, const double* t0, double prec, double* r) {
    const double sw = sqrt(prec);
    r[0] = sw * (lx - t0[0]); r[1] = sw * (ly - t0[1]);
    return sw;
}
// the cost; H holds the two diagonal entries, g 2.
SCORE_GN_HD double gn_prior_block(double lx, double ly, const double* t0, double prec, double* H, double* g) {
    double r[2];
    const double sw = gn_prior_jac(lx, ly, t0, prec, r);
    const double r0 = r[0], r1 = r[1];
    if (H) { H[0] = prec; H[1] = prec; g[0] = sw * r0; g[1] = sw * r1; }
    return r0 * r0 + r1 * r1;
}

// ---------------------------------------------------------------------------
// SE(3): state = [R_p (9, row-major), t_p (3)] for every pose p = 0..Np-1 (pose 0 stays where it is), then the
// landmarks (3 each).  Local unknowns of a pose: omega (R <- R Exp(omega)), v (t <- t + v).
// ---------------------------------------------------------------------------
SCORE_GN_HD void gn_so3_exp(const double* w, double* E) {  // Rodrigues; E row-major
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    const double th = sqrt(th2);
    double A, B;
    if (th < 1e-8) { A = 1.0 - th2 / 6.0; B = 0.5 - th2 / 24.0; }
    else { A = sin(th) / th; B = (1.0 - cos(th)) / th2; }
    const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0.0;
            for (int k = 0; k < 3; ++k) kk += K[i * 3 + k] * K[k * 3 + j];
            E[i * 3 + j] = (i == j ? 1.0 : 0.0) + A * K[i * 3 + j] + B * kk;
        }
}
// retraction of one pose: out = [R Exp(omega) | t + v]   (step == nullptr: copy)
SCORE_GN_HD void gn_pose3_retract(const double* X, const double* step, double* out) {
    if (!step) { for (int k = 0; k < 12; ++k) out[k] = X[k]; return; }
    double E[9];
    gn_so3_exp(step, E);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double a = 0.0;
            for (int k = 0; k < 3; ++k) a += X[i * 3 + k] * E[k * 3 + j];
            out[i * 3 + j] = a;
        }
    for (int k = 0; k < 3; ++k) out[9 + k] = X[9 + k] + step[3 + k];
}
// point of a range endpoint in the 3-D state
SCORE_GN_HD const double* gn_point3(const double* X, int64_t Np, int64_t v) {
    return v < Np ? X + 12 * v + 9 : X + 12 * Np + 3 * (v - Np);
}

// relative-pose measurement i -> j in 3-D.  Local unknowns [om_i, v_i, om_j, v_j] (12).  Residuals r (12):
// sqrt(kappa) (t_j - t_i - R_i tm), sqrt(tau) (R_j - R_i Rm) row-major; with_jac: J = dr/d(local unknowns), 12 x 12.
SCORE_GN_HD void gn_rel_jac3(const double* Xi, const double* Xj, const double* tm, const double* Rm, double kappa, double tau,
                             double* r, double (*J)[12], bool with_jac) {
    const double sk = sqrt(kappa), st = sqrt(tau);
    const double* Ri = Xi; const double* ti = Xi + 9;
    const double* Rj = Xj; const double* tj = Xj + 9;
    for (int a = 0; a < 3; ++a) {
        double rt = 0.0;
        for (int k = 0; k < 3; ++k) rt += Ri[a * 3 + k] * tm[k];
        r[a] = sk * (tj[a] - ti[a] - rt);
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double rr = 0.0;
            for (int k = 0; k < 3; ++k) rr += Ri[a * 3 + k] * Rm[k * 3 + b];
            r[3 + a * 3 + b] = st * (Rj[a * 3 + b] - rr);
        }
    if (!with_jac) return;
    // J (12 x 12): columns [om_i 0..2 | v_i 3..5 | om_j 6..8 | v_j 9..11]
    for (int a = 0; a < 12; ++a)
        for (int b = 0; b < 12; ++b) J[a][b] = 0.0;
    // translation rows: d/dv_j = I, d/dv_i = -I, d/dom_i = R_i [tm]x
    const double tx[9] = {0.0, -tm[2], tm[1], tm[2], 0.0, -tm[0], -tm[1], tm[0], 0.0};
    for (int a = 0; a < 3; ++a) {
        J[a][9 + a] = sk;
        J[a][3 + a] = -sk;
        for (int c = 0; c < 3; ++c) {
            double m = 0.0;
            for (int k = 0; k < 3; ++k) m += Ri[a * 3 + k] * tx[k * 3 + c];
            J[a][c] = sk * m;
        }
    }
    // rotation rows: d/dom_j[c] = R_j [e_c]x ; d/dom_i[c] = -R_i [e_c]x Rm
    for (int c = 0; c < 3; ++c) {
        double Ec[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        // [e_c]x : (e_c x) entries
        if (c == 0) { Ec[5] = -1.0; Ec[7] = 1.0; }
        else if (c == 1) { Ec[2] = 1.0; Ec[6] = -1.0; }
        else { Ec[1] = -1.0; Ec[3] = 1.0; }
        double RjE[9], RiE[9];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                double x = 0.0, y = 0.0;
                for (int k = 0; k < 3; ++k) { x += Rj[a * 3 + k] * Ec[k * 3 + b]; y += Ri[a * 3 + k] * Ec[k * 3 + b]; }
                RjE[a * 3 + b] = x; RiE[a * 3 + b] = y;
            }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                double y = 0.0;
                for (int k = 0; k < 3; ++k) y += RiE[a * 3 + k] * Rm[k * 3 + b];
                J[3 + a * 3 + b][6 + c] = st * RjE[a * 3 + b];
                J[3 + a * 3 + b][c] = -st * y;
            }
    }
}
// The curvature term in 3-D, in the coordinates of the retraction R Exp(omega): d^2 (R Exp omega) / d omega_a d omega_b at
// omega = 0 is R S_ab with S_ab = ([e_a]x [e_b]x + [e_b]x [e_a]x) / 2 = (e_a e_b' + e_b e_a') / 2 - delta_ab I, so for any N
// trace(S_ab N) = (N_ab + N_ba) / 2 - delta_ab trace N.  Only the (om_i, om_i) and (om_j, om_j) 3 x 3 sub-blocks of the
// 12 x 12 block H get a term:
//   (om_i, om_i)  -sqrt(kappa) r_t' R_i S_ab tm - sqrt(tau) <r_R, R_i S_ab Rm>  = -trace(S_ab N_i),  N_i = tm (R_i' r_t)' sqrt(kappa)
//                                                                                                   + Rm r_R' R_i sqrt(tau)
//   (om_j, om_j)  +sqrt(tau) <r_R, R_j S_ab>                                    = +trace(S_ab N_j),  N_j = r_R' R_j sqrt(tau)
// r: what gn_rel_jac3 gave at the point (r_t = r[0..2], r_R = r[3..11] row-major).
SCORE_GN_HD void gn_rel_curv3(const double* Xi, const double* Xj, const double* tm, const double* Rm, double kappa, double tau,
                              const double* r, double* H) {
    const double sk = sqrt(kappa), st = sqrt(tau);
    double u[3], A[9], Ni[9], Nj[9];  // u = R_i' r_t, A = r_R' R_i
    for (int a = 0; a < 3; ++a) {
        double s = 0.0;
        for (int k = 0; k < 3; ++k) s += Xi[k * 3 + a] * r[k];
        u[a] = s;
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double x = 0.0, y = 0.0;
            for (int k = 0; k < 3; ++k) { x += r[3 + k * 3 + a] * Xi[k * 3 + b]; y += r[3 + k * 3 + a] * Xj[k * 3 + b]; }
            A[a * 3 + b] = x;
            Nj[a * 3 + b] = st * y;
        }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            double x = 0.0;
            for (int k = 0; k < 3; ++k) x += Rm[a * 3 + k] * A[k * 3 + b];
            Ni[a * 3 + b] = sk * tm[a] * u[b] + st * x;
        }
    const double tri = Ni[0] + Ni[4] + Ni[8], trj = Nj[0] + Nj[4] + Nj[8];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            const double d = a == b ? 1.0 : 0.0;
            H[a * 12 + b] -= 0.5 * (Ni[a * 3 + b] + Ni[b * 3 + a]) - d * tri;
            H[(6 + a) * 12 + 6 + b] += 0.5 * (Nj[a * 3 + b] + Nj[b * 3 + a]) - d * trj;
        }
}
// the cost r'r; with H / g: J'J (12 x 12) and J'r; exact: H with the curvature term.
SCORE_GN_HD double gn_rel_block3(const double* Xi, const double* Xj, const double* tm, const double* Rm, double kappa, double tau,
                                 double* H, double* g, bool exact = false) {
    double r[12], J[12][12];
    gn_rel_jac3(Xi, Xj, tm, Rm, kappa, tau, r, J, H != nullptr);
    double cost = 0.0;
    for (int k = 0; k < 12; ++k) cost += r[k] * r[k];
    if (!H) return cost;
    gn_normal_products<12>(J, r, H, g);
    if (exact) gn_rel_curv3(Xi, Xj, tm, Rm, kappa, tau, r, H);
    return cost;
}

// range between points a and b in 3-D.  Local unknowns [pa (3), pb (3)].  Returns r; J (with_jac): its one row (6).
SCORE_GN_HD double gn_range_jac3(const double* pa, const double* pb, double dist, double prec, double* J, bool with_jac) {
    const double sw = sqrt(prec);
    const double d[3] = {pa[0] - pb[0], pa[1] - pb[1], pa[2] - pb[2]};
    const double rho = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const double r = sw * (rho - dist);
    if (with_jac) {
        const bool tiny = !(rho > 1e-12);
        for (int k = 0; k < 3; ++k) { J[k] = tiny ? 0.0 : sw * d[k] / rho; J[3 + k] = -J[k]; }
    }
    return r;
}
// the cost r'r; with H / g: H 6 x 6, g 6; exact: H with the curvature term.
SCORE_GN_HD double gn_range_block3(const double* pa, const double* pb, double dist, double prec, double* H, double* g,
                                   bool exact = false) {
    double J[6];
    const double r = gn_range_jac3(pa, pb, dist, prec, J, H != nullptr);
    if (H) {
        for (int a = 0; a < 6; ++a) {
            g[a] = J[a] * r;
            for (int b = 0; b < 6; ++b) H[a * 6 + b] = J[a] * J[b];
        }
        if (exact) {
            const double d[3] = {pa[0] - pb[0], pa[1] - pb[1], pa[2] - pb[2]};
            gn_range_curv<3>(d, prec, r, H);
        }
    }
    return r * r;
}

// landmark prior in 3-D.  r (3) = sqrt(prec) (l - t0); returns the Jacobian: sqrt(prec) times the identity.
SCORE_GN_HD double gn_prior_jac3(const double* l, const double* t0, double prec, double* r) {
    const double sw = sqrt(prec);
    for (int k = 0; k < 3; ++k) r[k] = sw * (l[k] - t0[k]);
    return sw;
}
// the cost; H holds the three diagonal entries, g 3.
SCORE_GN_HD double gn_prior_block3(const double* l, const double* t0, double prec, double* H, double* g) {
    double r3[3];
    const double sw = gn_prior_jac3(l, t0, prec, r3);
    double c = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double r = r3[k];
        c += r * r;
        if (H) { H[k] = prec; g[k] = sw * r; }
    }
    return c;
}

// The measurement arrays, stated once.  F<T> is how one array is held: a pointer (GnMeasPtr, what a lane reads), a host vector
// (GnMeas below), a device buffer (score_refine_handles.hpp).
template <template <class> class F>
struct GnMeasT {
    F<int32_t> rel_i, rel_j, rng_a, rng_b, pri_l;
    F<double> rel_t, rel_R, rel_kappa, rel_tau, rng_dist, rng_prec, pri_t, pri_prec;
};
template <class T> using GnConstPtr = const T*;
template <class T> using GnHostVec = std::vector<T>;
using GnMeasPtr = GnMeasT<GnConstPtr>;

// Every array of two forms side by side: f(a's, b's, family, width), family 0 the relative poses, 1 the ranges, 2 the landmark
// priors; an entry holds dim^width scalars.  Every conversion between the forms, and a member's offsets, go through this list.
template <class A, class B, class Fn>
SCORE_GN_HD void gn_meas_each(A& a, B& b, Fn&& f) {
    f(a.rel_i, b.rel_i, 0, 0); f(a.rel_j, b.rel_j, 0, 0); f(a.rng_a, b.rng_a, 1, 0); f(a.rng_b, b.rng_b, 1, 0); f(a.pri_l, b.pri_l, 2, 0);
    f(a.rel_t, b.rel_t, 0, 1); f(a.rel_R, b.rel_R, 0, 2); f(a.rel_kappa, b.rel_kappa, 0, 0); f(a.rel_tau, b.rel_tau, 0, 0);
    f(a.rng_dist, b.rng_dist, 1, 0); f(a.rng_prec, b.rng_prec, 1, 0); f(a.pri_t, b.pri_t, 2, 1); f(a.pri_prec, b.pri_prec, 2, 0);
}
// the table from entry rel0 / rng0 / pri0 of its families on: where a member of a union starts (score_gn_batch.hpp)
template <int DIM>
SCORE_GN_HD GnMeasPtr gn_meas_from(const GnMeasPtr& p, long long rel0, long long rng0, long long pri0) {
    const long long first[3] = {rel0, rng0, pri0};
    GnMeasPtr q;
    gn_meas_each(q, p, [&](auto& dst, const auto& src, int family, int width) {
        dst = src + (width == 0 ? 1 : width == 1 ? DIM : DIM * DIM) * first[family];
    });
    return q;
}

// ---------------------------------------------------------------------------
// One graph as a lane sees it, and what a lane does with one measurement / one variable of it: stated here once, compiled
// into the single handle's kernels (score_gn_kernels.hpp, score_gn_robust.hpp), the group's (score_gn_batch.hpp,
// score_gn_robust_batch.hpp: a workgroup's view is its member's) and the CPU twin's loops.
// ---------------------------------------------------------------------------
struct GnView {
    int64_t Np, Nl, n_rel, n_rng, n_pri;
    GnMeasPtr meas;        // the measurement arrays, from this graph's first entry
    const double* X;       // its state: every pose (2-D [theta, x, y], 3-D [R | t]), then the landmarks
    double *hblk, *gblk;   // its block storage: relative-pose blocks, then range blocks, then prior blocks
};

// dim as a compile-time constant: f(std::integral_constant<int, 2>) for dim == 2, <int, 3> otherwise (gn_build has refused
// every other value)
template <class F>
inline decltype(auto) gn_dim(int dim, F&& f) {
    if (dim == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 3>{});
}

// relative-pose entry m at the view's point with the precisions given: cost, with H / g also J'J (EXACT: with the curvature
// term, see gn_rel_curv) and J'r
template <int DIM, bool EXACT = false>
SCORE_GN_HD double gn_rel_at(const GnView& v, int64_t m, double kappa, double tau, double* H, double* g) {
    constexpr int PS = DIM == 2 ? 3 : 12;
    const double* pi = v.X + PS * (int64_t)v.meas.rel_i[m];
    const double* pj = v.X + PS * (int64_t)v.meas.rel_j[m];
    if (DIM == 2) return gn_rel_block(pi[0], pi[1], pi[2], pj[0], pj[1], pj[2], v.meas.rel_t + 2 * m, v.meas.rel_R + 4 * m, kappa, tau, H, g, EXACT);
    return gn_rel_block3(pi, pj, v.meas.rel_t + 3 * m, v.meas.rel_R + 9 * m, kappa, tau, H, g, EXACT);
}
// range r at the view's point with the precision given
template <int DIM, bool EXACT = false>
SCORE_GN_HD double gn_range_at(const GnView& v, int64_t r, double prec, double* H, double* g) {
    if (DIM == 2) {
        const double* pa = gn_point2(v.X, v.Np, v.meas.rng_a[r]);
        const double* pb = gn_point2(v.X, v.Np, v.meas.rng_b[r]);
        return gn_range_block(pa[0], pa[1], pb[0], pb[1], v.meas.rng_dist[r], prec, H, g, EXACT);
    }
    const double* pa = gn_point3(v.X, v.Np, v.meas.rng_a[r]);
    const double* pb = gn_point3(v.X, v.Np, v.meas.rng_b[r]);
    const double a3[3] = {pa[0], pa[1], pa[2]}, b3[3] = {pb[0], pb[1], pb[2]};
    return gn_range_block3(a3, b3, v.meas.rng_dist[r], prec, H, g, EXACT);
}

template <int N>
SCORE_GN_HD void gn_store(double* dst, const double* src) {
#pragma unroll
    for (int k = 0; k < N; ++k) dst[k] = src[k];
}

// measurement m of the view (relative poses, then ranges, then landmark priors; beyond them: nothing): its cost and,
// with_blocks, its J'J / J'r block into the view's storage (2-D 36 + 6 / 16 + 4 / 2 + 2 scalars, 3-D 144 + 12 / 36 + 6 / 3 + 3).
// EXACT: the block is that of E = J'J + sum_q r_q grad^2 r_q (half the Hessian of the cost), in the same layout; a landmark
// prior is linear and has no term.  A template argument, so that the Gauss-Newton instantiation is the code it was.
template <int DIM, bool EXACT = false>
SCORE_GN_HD double gn_measurement(const GnView& v, int64_t m, bool with_blocks) {
    constexpr int PS = DIM == 2 ? 3 : 12, NR = DIM == 2 ? 6 : 12, NG = 2 * DIM;
    double cost = 0.0;
    if (m < v.n_rel) {
        double H[NR * NR], g[NR];
        cost = gn_rel_at<DIM, EXACT>(v, m, v.meas.rel_kappa[m], v.meas.rel_tau[m], with_blocks ? H : nullptr, g);
        if (with_blocks) {
            double* ho = v.hblk + NR * NR * m;
            for (int k = 0; k < NR * NR; ++k) ho[k] = H[k];
            gn_store<NR>(v.gblk + NR * m, g);
        }
    } else if (m < v.n_rel + v.n_rng) {
        const int64_t r = m - v.n_rel;
        double H[NG * NG], g[NG];
        cost = gn_range_at<DIM, EXACT>(v, r, v.meas.rng_prec[r], with_blocks ? H : nullptr, g);
        if (with_blocks) {
            gn_store<NG * NG>(v.hblk + NR * NR * v.n_rel + NG * NG * r, H);
            gn_store<NG>(v.gblk + NR * v.n_rel + NG * r, g);
        }
    } else if (m < v.n_rel + v.n_rng + v.n_pri) {
        const int64_t e = m - v.n_rel - v.n_rng;
        const double* l = v.X + PS * v.Np + DIM * (int64_t)v.meas.pri_l[e];
        double H[DIM], g[DIM];
        if (DIM == 2) {
            cost = gn_prior_block(l[0], l[1], v.meas.pri_t + 2 * e, v.meas.pri_prec[e], with_blocks ? H : nullptr, g);
        } else {
            const double l3[3] = {l[0], l[1], l[2]};
            cost = gn_prior_block3(l3, v.meas.pri_t + 3 * e, v.meas.pri_prec[e], with_blocks ? H : nullptr, g);
        }
        if (with_blocks) {
            gn_store<DIM>(v.hblk + NR * NR * v.n_rel + NG * NG * v.n_rng + DIM * e, H);
            gn_store<DIM>(v.gblk + NR * v.n_rel + NG * v.n_rng + DIM * e, g);
        }
    }
    return cost;
}

// Residual of the robust refinement (include/score_refine_robust.h): r = sqrt(the measurement's own cost term) -- the block
// functions without H / g -- with the MEASURED precisions, which the caller passes.
//   kGnRobustRanges    range m:                sqrt(p0) | |p_a - p_b| - dist |
//   kGnRobustClosures  relative-pose entry m:  sqrt(p0 |t_j - t_i - R_i t~|^2 + p1 |R_j - R_i R~|_F^2)   (p0 = kappa, p1 = tau)
template <int DIM>
SCORE_GN_HD double gn_robust_residual(const GnView& v, int family, int64_t m, double p0, double p1) {
    return sqrt(family == kGnRobustRanges ? gn_range_at<DIM>(v, m, p0, nullptr, nullptr) : gn_rel_at<DIM>(v, m, p0, p1, nullptr, nullptr));
}

// variable i (pose or landmark) of a graph: dst = retract(src, step) -- a pose's step added (3-D: R Exp(omega), t + v), a
// landmark's added; step: the graph's first unknown, pose p >= 1 owns [DP (p - 1), DP p), the landmarks follow.  The copy:
// pose 0 (it has no unknowns), and every variable with step == nullptr.
template <int DIM>
SCORE_GN_HD void gn_retract_variable(const double* src, const double* step, double* dst, int64_t Np, int64_t Nl, int64_t i) {
    constexpr int PS = DIM == 2 ? 3 : 12, DP = DIM == 2 ? 3 : 6;
    if (i < Np) {
        const double* in = src + PS * i;
        double* out = dst + PS * i;
        if (!step || i == 0) {
            gn_store<PS>(out, in);
        } else if (DIM == 2) {
            const double* st = step + DP * (i - 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) out[k] = in[k] + st[k];
        } else {
            double a[12], s6[6], o[12];
            gn_store<12>(a, in);
            gn_store<6>(s6, step + DP * (i - 1));
            gn_pose3_retract(a, s6, o);
            gn_store<12>(out, o);
        }
    } else if (i < Np + Nl) {
        const int64_t l = i - Np;
        const double* in = src + PS * Np + DIM * l;
        double* out = dst + PS * Np + DIM * l;
        const double* st = step ? step + DP * (Np - 1) + DIM * l : nullptr;
#pragma unroll
        for (int k = 0; k < DIM; ++k) out[k] = st ? in[k] + st[k] : in[k];
    }
}

// Not used in this tree any more.  The 2-D state used to hold the unknowns alone, u = [theta, x, y of poses 1.. | landmarks],
// with pose 0 beside it in GnProblem::pin; these are that layout's accessors.  They and GnProblem::pin stay for one revision so
// that the CPU twin's previous source still builds against this header, and go with the next change here.
SCORE_GN_HD void gn_pose(const double* u, const double* pin, int64_t p, double& th, double& x, double& y) {
    if (p == 0) { th = pin[0]; x = pin[1]; y = pin[2]; return; }
    const double* q = u + 3 * (p - 1);
    th = q[0]; x = q[1]; y = q[2];
}
SCORE_GN_HD void gn_point(const double* u, const double* pin, int64_t Np, int64_t v, double& x, double& y) {
    if (v < Np) { double th; gn_pose(u, pin, v, th, x, y); return; }
    const double* q = u + 3 * (Np - 1) + 2 * (v - Np);
    x = q[0]; y = q[1];
}

// ---------------------------------------------------------------------------
// host side: the graph, the pattern of J'J, the contribution lists
// ---------------------------------------------------------------------------
struct GnMeas : GnMeasT<GnHostVec> {  // the measurement arrays on the host
    int64_t n_rel() const { return (int64_t)rel_i.size(); }
    int64_t n_rng() const { return (int64_t)rng_a.size(); }
    int64_t n_pri() const { return (int64_t)pri_l.size(); }
    void append(const GnMeas& o) {  // o's entries after these: a union grows by a member
        gn_meas_each(*this, o, [](auto& dst, const auto& src, int, int) { dst.insert(dst.end(), src.begin(), src.end()); });
    }
    GnMeasPtr ptrs() const {
        GnMeasPtr p;
        gn_meas_each(p, *this, [](auto& dst, const auto& src, int, int) { dst = src.data(); });
        return p;
    }
};

struct GnProblem : GnMeas {
    int dim = 2;
    int64_t Np = 0, Nl = 0, n = 0;
    int dp() const { return dim == 2 ? 3 : 6; }          // unknowns per pose
    int rel_nb() const { return 2 * dp(); }              // local unknowns of a relative-pose block
    int rng_nb() const { return 2 * dim; }
    int64_t state_size() const { return (dim == 2 ? 3 : 12) * Np + dim * Nl; }  // every pose (2-D [theta, x, y], 3-D [R | t]), landmarks
    std::vector<int32_t> chain_len;
    double pin[3] = {0, 0, 0};  // (not used any more: see gn_pose)
    // block storage: rel blocks (36 + 6 each), then range blocks (16 + 4), then prior blocks (2 + 2)
    int64_t hblk_size() const { return (int64_t)rel_nb() * rel_nb() * n_rel() + (int64_t)rng_nb() * rng_nb() * n_rng() + dim * n_pri(); }
    int64_t gblk_size() const { return (int64_t)rel_nb() * n_rel() + (int64_t)rng_nb() * n_rng() + dim * n_pri(); }
    int64_t n_meas() const { return n_rel() + n_rng() + n_pri(); }
    // pattern of H (CSR, sorted, with diagonal) and, per entry / per unknown, the block slots it sums
    std::vector<int32_t> hptr, hcol, hc_ptr, hc_slot, gc_ptr, gc_slot, diag_pos;
    std::vector<int32_t> chain_ptr, node_first_col;

    GnView view(const double* X, double* hblk, double* gblk) const {  // the graph from host memory
        return GnView{Np, Nl, n_rel(), n_rng(), n_pri(), ptrs(), X, hblk, gblk};
    }
    int64_t pose_col(int64_t p) const { return p == 0 ? -1 : dp() * (p - 1); }
    // first column of the translation of a range endpoint (2-D: after theta; 3-D: after omega)
    int64_t point_col(int64_t v) const { return v < Np ? (v == 0 ? -1 : dp() * (v - 1) + (dp() - dim)) : dp() * (Np - 1) + dim * (v - Np); }
};

// What the linear-mode handle behind a refinement is created from: the pattern of H alone (the gathers write its values) with
// the chain hint, 3 x 3 blocks.  The vectors must outlive the create.
inline score_problem gn_linear_pattern(int64_t n, const std::vector<int32_t>& hptr, const std::vector<int32_t>& hcol,
                                       const std::vector<int32_t>& chain_ptr, const std::vector<int32_t>& node_first_col) {
    score_problem pat{};
    pat.n = (int32_t)n; pat.m = 0;
    pat.P_rowptr = hptr.data(); pat.P_col = hcol.data();
    pat.block_size = 3; pat.n_chains = (int32_t)chain_ptr.size() - 1;
    pat.chain_ptr = chain_ptr.data(); pat.node_first_col = node_first_col.data();
    return pat;
}

inline void gn_build(const score_graph& g, GnProblem& P) {
    BuildScope scope;
    if (g.dim != 2 && g.dim != 3) throw std::runtime_error("score_refine: dim must be 2 or 3");
    if (g.n_chains <= 0 || !g.chain_len) throw std::runtime_error("score_refine: no pose chains");
    P.dim = g.dim;
    const int d = g.dim, dp = P.dp(), nbr = P.rel_nb(), nbg = P.rng_nb();
    P.chain_len.assign(g.chain_len, g.chain_len + g.n_chains);
    P.Np = 0;
    for (int c = 0; c < g.n_chains; ++c) {
        if (g.chain_len[c] < 0) throw std::runtime_error("score_refine: negative chain length");
        P.Np += g.chain_len[c];
    }
    if (P.Np == 0 || g.chain_len[0] == 0) throw std::runtime_error("score_refine: no pose variables");
    P.Nl = g.n_landmarks;
    P.n = (int64_t)dp * (P.Np - 1) + (int64_t)d * P.Nl;
    if (P.n >= ((int64_t)1 << 31) / 64) throw std::runtime_error("score_refine: too many unknowns");
    P.rel_i.assign(g.rel_base, g.rel_base + g.n_rel);
    P.rel_j.assign(g.rel_to, g.rel_to + g.n_rel);
    P.rel_t.assign(g.rel_t, g.rel_t + (int64_t)d * g.n_rel);
    P.rel_R.assign(g.rel_R, g.rel_R + (int64_t)d * d * g.n_rel);
    P.rel_kappa.assign(g.rel_kappa, g.rel_kappa + g.n_rel);
    P.rel_tau.assign(g.rel_tau, g.rel_tau + g.n_rel);
    P.rng_a.assign(g.rng_a, g.rng_a + g.n_rng);
    P.rng_b.assign(g.rng_b, g.rng_b + g.n_rng);
    P.rng_dist.assign(g.rng_dist, g.rng_dist + g.n_rng);
    P.rng_prec.assign(g.rng_prec, g.rng_prec + g.n_rng);
    P.pri_l.assign(g.lprior_lm, g.lprior_lm + g.n_lprior);
    P.pri_t.assign(g.lprior_t, g.lprior_t + (int64_t)d * g.n_lprior);
    P.pri_prec.assign(g.lprior_prec, g.lprior_prec + g.n_lprior);
    for (int64_t e = 0; e < g.n_rel; ++e)
        if (P.rel_i[e] < 0 || P.rel_i[e] >= P.Np || P.rel_j[e] < 0 || P.rel_j[e] >= P.Np)
            throw std::runtime_error("score_refine: relative-pose endpoint out of range");
    for (int64_t r = 0; r < g.n_rng; ++r)
        if (P.rng_a[r] < 0 || P.rng_a[r] >= P.Np + P.Nl || P.rng_b[r] < 0 || P.rng_b[r] >= P.Np + P.Nl)
            throw std::runtime_error("score_refine: range endpoint out of range");
    for (int64_t e = 0; e < g.n_lprior; ++e)
        if (P.pri_l[e] < 0 || P.pri_l[e] >= P.Nl) throw std::runtime_error("score_refine: landmark prior out of range");

    // Every block entry that lands on two unknowns is a (row, col, slot) triplet.  The measurement loops run
    // twice over the same code -- a counting pass sizes every row, a filling pass writes (col, slot) pairs in
    // measurement order -- then the rows are ordered by column and merged in parallel (stable: an entry sums
    // its slots in measurement order on every backend).  Gradient lists: the same without columns.
    const int64_t hb_rng = (int64_t)nbr * nbr * g.n_rel, gb_rng = (int64_t)nbr * g.n_rel;
    const int64_t hb_pri = hb_rng + (int64_t)nbg * nbg * g.n_rng, gb_pri = gb_rng + (int64_t)nbg * g.n_rng;
    std::vector<int32_t> hcnt((size_t)P.n + 1, 0), gcnt((size_t)P.n + 1, 0), hfill, gfill, tcol, tslot;
    bool filling = false;
    auto addH = [&](int64_t row, int64_t col, int64_t slot) {
        if (!filling) { ++hcnt[(size_t)row + 1]; return; }
        const int32_t pos = hfill[(size_t)row]++;
        tcol[(size_t)pos] = (int32_t)col;
        tslot[(size_t)pos] = (int32_t)slot;
    };
    auto addG = [&](int64_t row, int64_t slot) {
        if (!filling) { ++gcnt[(size_t)row + 1]; return; }
        P.gc_slot[(size_t)gfill[(size_t)row]++] = (int32_t)slot;
    };
    auto measurements = [&]() {
        for (int64_t e = 0; e < g.n_rel; ++e) {
            const int64_t ci = P.pose_col(P.rel_i[e]), cj = P.pose_col(P.rel_j[e]);
            int64_t L[12];
            for (int a = 0; a < dp; ++a) { L[a] = ci < 0 ? -1 : ci + a; L[dp + a] = cj < 0 ? -1 : cj + a; }
            for (int a = 0; a < nbr; ++a) {
                if (L[a] < 0) continue;
                addG(L[a], (int64_t)nbr * e + a);
                for (int b = 0; b < nbr; ++b)
                    if (L[b] >= 0) addH(L[a], L[b], (int64_t)nbr * nbr * e + a * nbr + b);
            }
        }
        for (int64_t r = 0; r < g.n_rng; ++r) {
            const int64_t ca = P.point_col(P.rng_a[r]), cb = P.point_col(P.rng_b[r]);
            int64_t L[6];
            for (int a = 0; a < d; ++a) { L[a] = ca < 0 ? -1 : ca + a; L[d + a] = cb < 0 ? -1 : cb + a; }
            for (int a = 0; a < nbg; ++a) {
                if (L[a] < 0) continue;
                addG(L[a], gb_rng + (int64_t)nbg * r + a);
                for (int b = 0; b < nbg; ++b)
                    if (L[b] >= 0) addH(L[a], L[b], hb_rng + (int64_t)nbg * nbg * r + a * nbg + b);
            }
        }
        for (int64_t e = 0; e < g.n_lprior; ++e) {
            const int64_t c = (int64_t)dp * (P.Np - 1) + (int64_t)d * (int64_t)P.pri_l[e];
            for (int a = 0; a < d; ++a) {
                addG(c + a, gb_pri + (int64_t)d * e + a);
                addH(c + a, c + a, hb_pri + (int64_t)d * e + a);
            }
        }
        for (int64_t i = 0; i < P.n; ++i) addH(i, i, -1);  // the diagonal always exists
    };
    measurements();  // counting pass
    for (int64_t i = 0; i < P.n; ++i) { hcnt[(size_t)i + 1] += hcnt[(size_t)i]; gcnt[(size_t)i + 1] += gcnt[(size_t)i]; }
    tcol.resize((size_t)hcnt[(size_t)P.n]); tslot.resize((size_t)hcnt[(size_t)P.n]);
    P.gc_ptr = gcnt;
    P.gc_slot.assign((size_t)gcnt[(size_t)P.n], 0);
    hfill.assign(hcnt.begin(), hcnt.end() - 1);
    gfill.assign(gcnt.begin(), gcnt.end() - 1);
    filling = true;
    measurements();  // filling pass
    // rows -> pattern + contribution lists, part by part
    struct Part { std::vector<int32_t> col, ent_len, slot, row_len; int64_t i0 = 0; };
    const int T = parallel_parts(P.n, 4096);
    std::vector<Part> parts((size_t)std::max(1, T));
    P.diag_pos.assign((size_t)P.n, -1);
    std::vector<int32_t> diag_rel((size_t)P.n, -1);  // position of the diagonal within its part
    auto row_weight = [&](int64_t i) {
        const double w = (double)(hcnt[(size_t)i + 1] - hcnt[(size_t)i]);
        return w > 64.0 ? 4.0 * w : w;
    };
    parallel_ranges_balanced(P.n, 4096, row_weight, [&](int t, int64_t i0, int64_t i1) {
        Part W;
        W.i0 = i0;
        W.col.reserve((size_t)(hcnt[(size_t)i1] - hcnt[(size_t)i0]));
        W.slot.reserve((size_t)(hcnt[(size_t)i1] - hcnt[(size_t)i0]));
        struct Ent { int32_t col, slot; };
        std::vector<Ent> L;
        for (int64_t i = i0; i < i1; ++i) {
            L.clear();
            for (int32_t k = hcnt[(size_t)i]; k < hcnt[(size_t)i + 1]; ++k) L.push_back(Ent{tcol[(size_t)k], tslot[(size_t)k]});
            if (L.size() > 64) {
                std::stable_sort(L.begin(), L.end(), [](const Ent& x, const Ent& y) { return x.col < y.col; });
            } else {
                for (size_t x = 1; x < L.size(); ++x) {
                    const Ent e = L[x];
                    size_t y = x;
                    while (y > 0 && L[y - 1].col > e.col) { L[y] = L[y - 1]; --y; }
                    L[y] = e;
                }
            }
            int32_t nent = 0;
            size_t k = 0;
            while (k < L.size()) {
                const int32_t col = L[k].col;
                int32_t ns = 0;
                if (col == (int32_t)i) diag_rel[(size_t)i] = (int32_t)W.col.size();
                for (; k < L.size() && L[k].col == col; ++k)
                    if (L[k].slot >= 0) { W.slot.push_back(L[k].slot); ++ns; }
                W.col.push_back(col);
                W.ent_len.push_back(ns);
                ++nent;
            }
            W.row_len.push_back(nent);
        }
        parts[(size_t)t] = std::move(W);
    }, T);
    {
        std::vector<size_t> eoff(parts.size() + 1, 0), soff(parts.size() + 1, 0);
        for (size_t k = 0; k < parts.size(); ++k) {
            eoff[k + 1] = eoff[k] + parts[k].col.size();
            soff[k + 1] = soff[k] + parts[k].slot.size();
        }
        P.hptr.assign((size_t)P.n + 1, 0);
        P.hcol.resize(eoff.back());
        P.hc_ptr.assign(eoff.back() + 1, 0);
        P.hc_slot.resize(soff.back());
        parallel_ranges((int64_t)parts.size(), 1, [&](int, int64_t k0, int64_t k1) {
            for (int64_t k = k0; k < k1; ++k) {
                const Part& W = parts[(size_t)k];
                std::copy(W.col.begin(), W.col.end(), P.hcol.begin() + (std::ptrdiff_t)eoff[(size_t)k]);
                std::copy(W.slot.begin(), W.slot.end(), P.hc_slot.begin() + (std::ptrdiff_t)soff[(size_t)k]);
                int32_t acc = (int32_t)eoff[(size_t)k];
                for (size_t r = 0; r < W.row_len.size(); ++r) {
                    const int64_t i = W.i0 + (int64_t)r;
                    P.diag_pos[(size_t)i] = (int32_t)eoff[(size_t)k] + diag_rel[(size_t)i];
                    acc += W.row_len[r];
                    P.hptr[(size_t)i + 1] = acc;
                }
                int32_t sacc = (int32_t)soff[(size_t)k];
                for (size_t e = 0; e < W.ent_len.size(); ++e) { sacc += W.ent_len[e]; P.hc_ptr[eoff[(size_t)k] + e + 1] = sacc; }
            }
        });
    }
    // chain hint (3 x 3 blocks).  2-D: one chain per robot, node = pose (theta, x, y).  3-D: two chains per robot,
    // the omega blocks and the v blocks of its poses (columns 6 (p - 1) and 6 (p - 1) + 3).  The pinned pose is not a node.
    P.chain_ptr.assign(1, 0);
    P.node_first_col.clear();
    const int kinds = d == 2 ? 1 : 2;
    int64_t p0 = 0;
    for (int c = 0; c < g.n_chains; ++c) {
        for (int kind = 0; kind < kinds; ++kind) {
            int32_t nodes = 0;
            for (int32_t i = 0; i < g.chain_len[c]; ++i) {
                const int64_t p = p0 + i;
                if (p == 0) continue;
                P.node_first_col.push_back((int32_t)(dp * (p - 1) + 3 * kind));
                ++nodes;
            }
            if (nodes > 0) P.chain_ptr.push_back(P.chain_ptr.back() + nodes);
        }
        p0 += g.chain_len[c];
    }
}

}  // namespace score

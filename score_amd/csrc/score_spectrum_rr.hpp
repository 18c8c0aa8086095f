// score_spectrum_rr.hpp -- the host half of the block eigensolver (score_spectrum.hpp): Rayleigh-Ritz on the pencil
// (S'AS, S'S) of the trial basis S = [X | W | P].  Nothing of the backend is used here: <cmath>, <vector> and plain loops, so
// the file compiles alone (tests/tools/spectrum_rr_check.cpp builds it with the host sanitizers).  No LAPACK is linked: the
// matrices are 48 x 48, and two cyclic Jacobi eigen-decompositions of that size cost well under a millisecond.
//
//   1. symmetrise both matrices; a direction whose Gram diagonal is zero, negative or non-finite is not in use (a done
//      column's W and P, the P block of the first iteration) and gets zero coefficients;
//   2. scale the pencil by the Gram diagonal, D = diag(B)^-1/2: the columns of S differ by many orders of magnitude (a
//      residual near convergence against a unit Ritz vector), the scaled Gram matrix has a unit diagonal;
//   3. eigen-decompose the scaled Gram matrix, D B D = Q L Q', and drop the directions with L <= kSpRrDrop * max L: what is
//      left of them is rounding, and 1 / L would multiply it into the reduced problem;
//   4. solve the reduced symmetric problem T = L^-1/2 Q' (D A D) Q L^-1/2 by cyclic Jacobi, take the nb lowest pairs, and
//      map them back: C = D Q L^-1/2 Z.  Every column is rescaled to c'Bc = 1 and its value recomputed as the Rayleigh
//      quotient c'Ac of the UNSCALED matrices, so that what the residual kernel subtracts is the quotient of the vector that
//      the combine kernel actually forms;
//   5. a pencil that is non-finite, leaves fewer than nb directions, or has a non-positive lowest value (A = H + sigma I is
//      positive definite: anything else is rounding gone wrong) is tried once more without the P block; then breakdown.
//      `indefinite` lifts exactly the test of the lowest value: the pencil of an indefinite A (score_curvature.hpp: half the
//      Hessian of the cost) has negative Ritz values by right, and nothing else of the step reads their sign.
#pragma once

#include <cmath>
#include <vector>

namespace score {

constexpr double kSpRrDrop = 1e-10;  // relative to the largest eigenvalue of the scaled Gram matrix
constexpr int kSpRrOk = 0, kSpRrNoP = 1, kSpRrBreakdown = 2;

// Eigen-decomposition of the symmetric m x m matrix a (row-major, destroyed) by cyclic Jacobi: values w (ascending), vectors
// as the COLUMNS of v (row-major m x m).  Returns false where an entry is not finite.
inline bool sp_jacobi_eigh(int m, std::vector<double>& a, std::vector<double>& w, std::vector<double>& v) {
    const size_t M = (size_t)m;
    v.assign(M * M, 0.0);
    for (size_t i = 0; i < M; ++i) v[i * M + i] = 1.0;
    for (size_t i = 0; i < M * M; ++i)
        if (!std::isfinite(a[i])) return false;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (size_t p = 0; p < M; ++p) {
            diag += a[p * M + p] * a[p * M + p];
            for (size_t q = p + 1; q < M; ++q) off += a[p * M + q] * a[p * M + q];
        }
        if (off == 0.0 || off <= 1e-34 * diag) break;
        for (size_t p = 0; p + 1 < M; ++p)
            for (size_t q = p + 1; q < M; ++q) {
                const double apq = a[p * M + q];
                if (apq == 0.0) continue;
                const double app = a[p * M + p], aqq = a[q * M + q];
                if (std::fabs(apq) <= 1e-300 || std::fabs(apq) < 1e-20 * std::sqrt(std::fabs(app) * std::fabs(aqq))) {
                    a[p * M + q] = a[q * M + p] = 0.0;
                    continue;
                }
                const double tau = (aqq - app) / (2.0 * apq);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (size_t k = 0; k < M; ++k) {  // columns p, q
                    const double akp = a[k * M + p], akq = a[k * M + q];
                    a[k * M + p] = c * akp - s * akq;
                    a[k * M + q] = s * akp + c * akq;
                }
                for (size_t k = 0; k < M; ++k) {  // rows p, q
                    const double apk = a[p * M + k], aqk = a[q * M + k];
                    a[p * M + k] = c * apk - s * aqk;
                    a[q * M + k] = s * apk + c * aqk;
                }
                a[p * M + q] = a[q * M + p] = 0.0;
                for (size_t k = 0; k < M; ++k) {
                    const double vkp = v[k * M + p], vkq = v[k * M + q];
                    v[k * M + p] = c * vkp - s * vkq;
                    v[k * M + q] = s * vkp + c * vkq;
                }
            }
    }
    w.resize(M);
    for (size_t i = 0; i < M; ++i) w[i] = a[i * M + i];
    // ascending, by selection (m is small); the columns of v follow
    for (size_t i = 0; i + 1 < M; ++i) {
        size_t lo = i;
        for (size_t j = i + 1; j < M; ++j)
            if (w[j] < w[lo]) lo = j;
        if (lo != i) {
            const double t = w[i]; w[i] = w[lo]; w[lo] = t;
            for (size_t k = 0; k < M; ++k) { const double u = v[k * M + i]; v[k * M + i] = v[k * M + lo]; v[k * M + lo] = u; }
        }
    }
    for (size_t i = 0; i < M; ++i)
        if (!std::isfinite(w[i])) return false;
    return true;
}

// One attempt on the directions `use` (m flags).  theta: nb.  C: m x nb row-major.  kept: directions left after step 3.
inline bool sp_rr_attempt(int m, int nb, const double* GA, const double* GB, const std::vector<char>& use, double* theta, double* C,
                          int* kept, bool indefinite = false) {
    const size_t M = (size_t)m;
    std::vector<int> idx;
    std::vector<double> d;
    for (int i = 0; i < m; ++i) {
        const double b = GB[(size_t)i * M + (size_t)i];
        if (use[(size_t)i] && std::isfinite(b) && b > 0.0) { idx.push_back(i); d.push_back(1.0 / std::sqrt(b)); }
    }
    const size_t ma = idx.size();
    *kept = 0;
    if ((int)ma < nb) return false;
    std::vector<double> As(ma * ma), Bs(ma * ma), A0(ma * ma), B0(ma * ma);
    for (size_t i = 0; i < ma; ++i)
        for (size_t j = 0; j < ma; ++j) {
            const size_t ij = (size_t)idx[i] * M + (size_t)idx[j], ji = (size_t)idx[j] * M + (size_t)idx[i];
            A0[i * ma + j] = 0.5 * (GA[ij] + GA[ji]);
            B0[i * ma + j] = 0.5 * (GB[ij] + GB[ji]);
            As[i * ma + j] = A0[i * ma + j] * d[i] * d[j];
            Bs[i * ma + j] = B0[i * ma + j] * d[i] * d[j];
        }
    std::vector<double> lam, Q, scratch = Bs;
    if (!sp_jacobi_eigh((int)ma, scratch, lam, Q)) return false;
    const double lmax = lam[ma - 1];
    if (!(lmax > 0.0)) return false;
    size_t first = 0;
    while (first < ma && !(lam[first] > kSpRrDrop * lmax)) ++first;
    const size_t mk = ma - first;
    *kept = (int)mk;
    if ((int)mk < nb) return false;
    // Y = Q[:, first:] L^-1/2 (ma x mk); T = Y' As Y
    std::vector<double> Y(ma * mk), AY(ma * mk), T(mk * mk);
    for (size_t i = 0; i < ma; ++i)
        for (size_t j = 0; j < mk; ++j) Y[i * mk + j] = Q[i * ma + first + j] / std::sqrt(lam[first + j]);
    for (size_t i = 0; i < ma; ++i)
        for (size_t j = 0; j < mk; ++j) {
            double s = 0.0;
            for (size_t k = 0; k < ma; ++k) s += As[i * ma + k] * Y[k * mk + j];
            AY[i * mk + j] = s;
        }
    for (size_t i = 0; i < mk; ++i)
        for (size_t j = i; j < mk; ++j) {
            double s = 0.0;
            for (size_t k = 0; k < ma; ++k) s += Y[k * mk + i] * AY[k * mk + j];
            T[i * mk + j] = T[j * mk + i] = s;
        }
    std::vector<double> mu, Z;
    if (!sp_jacobi_eigh((int)mk, T, mu, Z)) return false;
    if (!indefinite && !(mu[0] > 0.0)) return false;
    for (size_t i = 0; i < M * (size_t)nb; ++i) C[i] = 0.0;
    std::vector<double> c(ma), t(ma);
    for (int j = 0; j < nb; ++j) {
        for (size_t i = 0; i < ma; ++i) {
            double s = 0.0;
            for (size_t k = 0; k < mk; ++k) s += Y[i * mk + k] * Z[k * mk + (size_t)j];
            c[i] = s * d[i];
        }
        double cbc = 0.0, cac = 0.0;
        for (size_t i = 0; i < ma; ++i) {
            double sb = 0.0, sa = 0.0;
            for (size_t k = 0; k < ma; ++k) { sb += B0[i * ma + k] * c[k]; sa += A0[i * ma + k] * c[k]; }
            cbc += c[i] * sb; cac += c[i] * sa;
        }
        if (!(cbc > 0.0) || !std::isfinite(cbc) || !std::isfinite(cac)) return false;
        const double sc = 1.0 / std::sqrt(cbc);
        theta[j] = cac / cbc;
        for (size_t i = 0; i < ma; ++i) C[(size_t)idx[i] * (size_t)nb + (size_t)j] = c[i] * sc;
    }
    return true;
}

// The nb lowest Ritz pairs of the pencil (GA, GB), both m x m row-major with m = 3 nb ([X | W | P]).  theta: nb ascending
// (up to the Rayleigh correction of step 4).  C: m x nb row-major.  Returns kSpRrOk, kSpRrNoP (the P block was left out: the
// caller's next P is what C says, as always) or kSpRrBreakdown (theta and C are not to be used).
inline int sp_rayleigh_ritz(int m, int nb, const double* GA, const double* GB, double* theta, double* C, int* kept,
                            bool indefinite = false) {
    std::vector<char> use((size_t)m, 1);
    int k = 0;
    if (sp_rr_attempt(m, nb, GA, GB, use, theta, C, &k, indefinite)) { if (kept) *kept = k; return kSpRrOk; }
    for (int i = 2 * nb; i < m; ++i) use[(size_t)i] = 0;
    if (sp_rr_attempt(m, nb, GA, GB, use, theta, C, &k, indefinite)) { if (kept) *kept = k; return kSpRrNoP; }
    if (kept) *kept = k;
    return kSpRrBreakdown;
}

}  // namespace score

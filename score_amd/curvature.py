"""The second-order check of a refined estimate (include/score_curvature.h).

``marginal_covariances``, ``information_spectrum``, ``posterior_samples`` and ``range_leverage`` read the Gauss-Newton
matrix J'J, which is positive semidefinite at every point: they cannot say whether the point the local solver stopped at is
a minimum.  Half the Hessian of the cost F = r'r,

    E = J'J + sum_q r_q grad^2 r_q          (q over the whitened residual rows),

can: a negative eigenvalue is a direction along which the cost falls to second order (a saddle -- ``Curvature.kind``,
``Curvature.negative``, and ``escape`` to leave it), and at a minimum E is the observed information, which differs from J'J
where the residuals are not small (``Curvature.gauss_newton``: v'(J'J)v beside every eigenvalue of E).  The unknowns are the
refinement's: (theta, x, y) per 2-D pose, (omega, v) of the retraction R Exp(omega), t + v per 3-D pose -- E is the Hessian
in those coordinates --, the coordinates of a landmark, the first pose fixed.

The curvature term of each measurement kind (csrc/score_gn.hpp states it for the device; here vectorised in NumPy):

  relative pose, 2-D   only (theta_i, theta_i) and (theta_j, theta_j): d^2 R / d theta^2 = -R, and the residual is
                       additively separable in i and j
  relative pose, 3-D   only the (omega_i, omega_i) and (omega_j, omega_j) 3 x 3 blocks: d^2 (R Exp omega) / d omega_a d omega_b
                       at 0 is R S_ab, S_ab = ([e_a]x [e_b]x + [e_b]x [e_a]x) / 2, and trace(S_ab N) = (N_ab + N_ba) / 2 -
                       delta_ab trace N
  range                r sqrt(prec) (I - u u') / rho on (a, a) and (b, b), the opposite sign on (a, b) and (b, a); zero where
                       rho <= 1e-12, as the Jacobian
  landmark prior       none

``hessian_spectrum`` runs the block eigensolver of ``information_spectrum`` on E + sigma I on the device
(``score_refine_curvature``) with the preconditioner of J'J + sigma I; ``engine="python"`` is the dense ``eigh`` of
``dense_hessian``: for small graphs, the tests, and libraries without the symbols.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import scipy.sparse as sp

from .bindings import CURVATURE, ScoreCurvatureInfo, ptr
from .marginals import _problem_and_point, _select
from .refine import _as_results, _point_arrays, _Problem3D
from .spectrum import MAX_MODES, MIN_DEVICE_UNKNOWNS, Modes, SpectrumHandle, _layout

# the symbols include/score_curvature.h declares
CURVATURE_SYMBOLS = list(CURVATURE)


# ---------------------------------------------------------------------------------------------------------------------
# E on the host
# ---------------------------------------------------------------------------------------------------------------------
class _Triplets:
    """(row, column, value) lists; an entry with a negative row or column belongs to the fixed pose and is dropped."""

    def __init__(self):
        self.rows, self.cols, self.vals = [], [], []

    def add(self, r, c, v):
        r, c, v = np.broadcast_arrays(np.asarray(r), np.asarray(c), np.asarray(v, dtype=np.float64))
        keep = (r >= 0) & (c >= 0)
        self.rows.append(r[keep].ravel()); self.cols.append(c[keep].ravel()); self.vals.append(v[keep].ravel())

    def matrix(self, n):
        if not self.rows:
            return sp.csr_matrix((n, n))
        return sp.csr_matrix((np.concatenate(self.vals), (np.concatenate(self.rows), np.concatenate(self.cols))), shape=(n, n))


def _range_terms(T, dv, r, sw, ca, cb):
    """r sqrt(prec) (I - u u') / rho of every range, on (a, a), (b, b) and, negated, on (a, b), (b, a).  ca, cb: the first
    column of each endpoint's point (negative: the fixed pose)."""
    d = dv.shape[1]
    rho = np.sqrt(np.einsum("ij,ij->i", dv, dv))
    ok = rho > 1e-12
    safe = np.where(ok, rho, 1.0)
    u = dv / safe[:, None]
    B = np.where(ok, r * sw / safe, 0.0)[:, None, None] * (np.eye(d)[None] - u[:, :, None] * u[:, None, :])
    NEG = -(10 ** 9)
    ca, cb = np.where(ca >= 0, ca, NEG), np.where(cb >= 0, cb, NEG)
    for a in range(d):
        for b in range(d):
            T.add(ca + a, ca + b, B[:, a, b]); T.add(cb + a, cb + b, B[:, a, b])
            T.add(ca + a, cb + b, -B[:, a, b]); T.add(cb + a, ca + b, -B[:, a, b])


def _curvature_2d(prob, u) -> sp.csr_matrix:
    th, t, lm = prob.split(u)
    c, s = np.cos(th), np.sin(th)
    bi, tj = prob.bi, prob.tj
    ne = len(bi)
    Ri = np.stack([c[bi], -s[bi], s[bi], c[bi]], axis=1).reshape(ne, 2, 2)
    Rj = np.stack([c[tj], -s[tj], s[tj], c[tj]], axis=1).reshape(ne, 2, 2)
    Rt = np.einsum("eij,ej->ei", Ri, prob.tm)
    RR = Ri @ prob.Rm
    rt = prob.sk[:, None] * (t[tj] - t[bi] - Rt)            # the whitened residual rows
    rR = prob.st[:, None, None] * (Rj - RR)
    # d^2 r_t / d theta_i^2 = +sqrt(kappa) R_i tm, d^2 r_R / d theta_i^2 = +sqrt(tau) R_i Rm, d^2 r_R / d theta_j^2 = -sqrt(tau) R_j
    hi = prob.sk * np.einsum("ei,ei->e", rt, Rt) + prob.st * np.einsum("eij,eij->e", rR, RR)
    hj = -prob.st * np.einsum("eij,eij->e", rR, Rj)
    T = _Triplets()
    ci, cj = prob._col_pose(bi), prob._col_pose(tj)
    T.add(ci, ci, hi); T.add(cj, cj, hj)
    dv = prob._point(prob.ra, t, lm) - prob._point(prob.rb, t, lm)
    r = prob.sw * (np.sqrt(np.einsum("ij,ij->i", dv, dv)) - prob.dist)
    _range_terms(T, dv, r, prob.sw, prob._col_point(prob.ra), prob._col_point(prob.rb))
    return T.matrix(prob.n)


def _sym_minus_trace(N):
    """trace(S_ab N) for every (a, b): (N + N') / 2 - trace(N) I, for a stack of 3 x 3 matrices."""
    return 0.5 * (N + np.swapaxes(N, 1, 2)) - np.trace(N, axis1=1, axis2=2)[:, None, None] * np.eye(3)[None]


def _curvature_3d(prob, state) -> sp.csr_matrix:
    R, t, lm = state
    bi, tj = prob.bi, prob.tj
    Ri, Rj = R[bi], R[tj]
    rt = prob.sk[:, None] * (t[tj] - t[bi] - np.einsum("eij,ej->ei", Ri, prob.tm))
    rR = prob.st[:, None, None] * (Rj - Ri @ prob.Rm)
    rRt = np.swapaxes(rR, 1, 2)
    u = np.einsum("eji,ej->ei", Ri, rt)                      # R_i' r_t
    Ni = prob.sk[:, None, None] * prob.tm[:, :, None] * u[:, None, :] + prob.st[:, None, None] * (prob.Rm @ (rRt @ Ri))
    Nj = prob.st[:, None, None] * (rRt @ Rj)
    Bi, Bj = -_sym_minus_trace(Ni), _sym_minus_trace(Nj)
    T = _Triplets()
    NEG = -(10 ** 9)
    ci, cj = np.where(bi > 0, 6 * (bi - 1), NEG), np.where(tj > 0, 6 * (tj - 1), NEG)
    for a in range(3):
        for b in range(3):
            T.add(ci + a, ci + b, Bi[:, a, b]); T.add(cj + a, cj + b, Bj[:, a, b])

    def pcol(v):
        pose = v < prob.Np
        return np.where(pose, np.where(v > 0, 6 * (v - 1) + 3, NEG), 6 * (prob.Np - 1) + 3 * (v - prob.Np))

    dv = prob._point(prob.ra, t, lm) - prob._point(prob.rb, t, lm)
    r = prob.sw * (np.linalg.norm(dv, axis=1) - prob.dist)
    _range_terms(T, dv, r, prob.sw, pcol(prob.ra), pcol(prob.rb))
    return T.matrix(prob.n)


def curvature_term(prob, point) -> sp.csr_matrix:
    """sum_q r_q grad^2 r_q at the point, sparse (duplicates summed)."""
    return _curvature_3d(prob, point) if isinstance(prob, _Problem3D) else _curvature_2d(prob, point)


def sparse_hessian(prob, point) -> sp.csr_matrix:
    """E = J'J + the curvature term at the point, sparse, on the pattern of J'J."""
    _, J = prob.residuals(point, jac=True)
    return ((J.T @ J) + curvature_term(prob, point)).tocsr()


def dense_hessian(prob, point) -> np.ndarray:
    """E at the point as a dense matrix (small graphs, tests): J'J of ``_Problem`` / ``_Problem3D`` plus the analytic
    curvature term."""
    return np.asarray(sparse_hessian(prob, point).todense(), dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the result
# ---------------------------------------------------------------------------------------------------------------------
class Curvature(Modes):
    """The k lowest eigenpairs of E (``Modes``: ``values`` may be negative; ``residuals`` are |E v_j - lambda_j v_j|_2).
    ``gauss_newton`` (k): v_j'(J'J)v_j, what the Gauss-Newton matrix holds along the same direction; ``h_max``: max diag J'J."""

    def __init__(self, values, vectors, residuals, gauss_newton, names, first, size, h_max, rel_tol, default_variables):
        super().__init__(values, vectors, residuals, names, first, size, h_max, rel_tol, default_variables)
        self.gauss_newton = np.asarray(gauss_newton, dtype=np.float64)

    def negative(self):
        """[(j, lambda_j, [(name, share), ...] by descending share)] for every mode with lambda_j < -rel_tol * h_max: the cost
        falls along v_j."""
        out = []
        for j in np.nonzero(self.values < -self.rel_tol * self.h_max)[0]:
            shares = sorted(((nm, float(p[j])) for nm, p in self.participation.items()), key=lambda e: -e[1])
            out.append((int(j), float(self.values[j]), shares))
        return out

    @property
    def kind(self) -> str:
        """"minimum": the lowest value is above rel_tol * h_max; "saddle": some value is below -rel_tol * h_max; "flat":
        neither -- the lowest value is not distinguishable from zero at the accuracy asked for."""
        tol = self.rel_tol * self.h_max
        if np.any(self.values < -tol):
            return "saddle"
        return "minimum" if self.values[0] > tol else "flat"


# ---------------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------------
class CurvatureHandle(SpectrumHandle):
    """A refinement handle kept for several ``score_refine_hessian_product`` / ``score_refine_curvature`` calls on one graph;
    every call of the handles it extends gives what it gave before one of these."""

    headers = SpectrumHandle.headers + (CURVATURE,)

    def product(self, point, V, exact=True):
        """A V with A = E (``exact``) or J'J at the point.  ``V``: n x c, c in 1..16 (or a vector); the result has its shape."""
        prob = self.prob
        poses, lms = _point_arrays(prob, point)
        V = np.asarray(V, dtype=np.float64)
        cols = V.reshape(prob.n, -1) if V.ndim == 1 else V
        if cols.ndim != 2 or cols.shape[0] != prob.n:
            raise ValueError(f"product: V must have {prob.n} rows")
        Vt = np.ascontiguousarray(cols.T)
        out = np.full_like(Vt, np.nan)
        rc = self.lib.score_refine_hessian_product(self.h, ptr(poses), ptr(lms), 1 if exact else 0, ptr(Vt), Vt.shape[0], ptr(out))
        if rc != 0:
            raise RuntimeError(f"score_refine_hessian_product failed: {self.lib.score_last_error().decode()}")
        return np.ascontiguousarray(out.T).reshape(V.shape)

    def curvature(self, point, k, rel_tol=1e-9, max_iters=200, shift=1e-8):
        """``score_refine_curvature`` as it is: (return code, values (k), vectors (k x n), residuals (k), v'(J'J)v (k), info
        record)."""
        prob = self.prob
        poses, lms = _point_arrays(prob, point)
        kk = max(0, min(int(k), MAX_MODES))
        values = np.full(kk, np.nan)
        vectors = np.full((kk, prob.n), np.nan)
        res = np.full(kk, np.nan)
        gn = np.full(kk, np.nan)
        info = ScoreCurvatureInfo()
        rc = self.lib.score_refine_curvature(self.h, ptr(poses), ptr(lms), int(k), float(rel_tol), int(max_iters), float(shift),
                                             ptr(values), ptr(vectors), ptr(res), ptr(gn), C.byref(info))
        if rc < 0:
            raise RuntimeError(f"score_refine_curvature failed: {self.lib.score_last_error().decode()}")
        return rc, values, vectors, res, gn, info.as_dict()


def device_curvature(prob, point, k, rel_tol=1e-9, max_iters=200, shift=1e-8, lib_path=None, solver_settings=None):
    """One ``CurvatureHandle.curvature`` call on a handle of its own."""
    with CurvatureHandle(prob, lib_path, solver_settings) as h:
        return h.curvature(point, k, rel_tol, max_iters, shift)


def _python_curvature(prob, point, k):
    _, J = prob.residuals(point, jac=True)
    H = (J.T @ J).tocsr()
    E = np.asarray((H + curvature_term(prob, point)).todense(), dtype=np.float64)
    w, V = np.linalg.eigh(0.5 * (E + E.T))
    w, V = w[:k], V[:, :k]
    res = np.linalg.norm(E @ V - V * w, axis=0)
    gn = np.einsum("ij,ij->j", V, H @ V)
    return w, V, res, gn, float(H.diagonal().max()), float(np.max(np.abs(E - H.todense())))


def hessian_spectrum(data, results, k: int = 8, range_weights=None, loop_closure_weights=None, rel_tol: float = 1e-9,
                     max_iters: int = 200, shift: float = 1e-8, engine: str = "device", lib_path: Optional[str] = None,
                     solver_settings: Optional[dict] = None):
    """The ``k`` (1..16) lowest eigenpairs of E, half the Hessian of the cost, at the estimate ``results`` -- normally what
    ``refine_estimate`` returned, with the same weights.  Returns ``(Curvature, info)``; ``info``: ``h_max`` (max diag J'J),
    ``shift`` (sigma = shift * h_max: the iteration runs on E + sigma I with the preconditioner of J'J + sigma I), ``c_max``
    (the largest entry of |E - J'J|), ``iterations``, ``unconverged``, ``setup_ms``, ``solve_ms``, ``engine``.  A pair counts
    as converged at |E v - lambda v|_2 <= rel_tol * h_max; one that is not raises RuntimeError naming the mode and its
    residual."""
    if engine not in ("device", "python"):
        raise ValueError("engine must be 'device' or 'python'")
    if int(k) != k or not 1 <= int(k) <= MAX_MODES:
        raise ValueError(f"k must be an integer in 1..{MAX_MODES}")
    if not rel_tol > 0 or not np.isfinite(rel_tol):
        raise ValueError("rel_tol must be positive")
    if int(max_iters) != max_iters or max_iters < 1:
        raise ValueError("max_iters must be at least 1")
    if not shift > 0 or not np.isfinite(shift):
        raise ValueError("shift must be positive")
    k = int(k)
    prob, point = _problem_and_point(data, results, range_weights, loop_closure_weights)
    if k > prob.n:
        raise ValueError(f"k = {k} modes of a graph with {prob.n} unknowns")
    names, first, size = _layout(prob)
    if engine == "python":
        values, V, res, gn, h_max, c_max = _python_curvature(prob, point, k)
        rec = {"h_max": h_max, "shift": shift * h_max, "c_max": c_max, "iterations": 0, "unconverged": 0, "setup_ms": 0.0,
               "solve_ms": 0.0}
    else:
        if prob.n < MIN_DEVICE_UNKNOWNS:
            raise ValueError(f"hessian_spectrum: {prob.n} unknowns are fewer than the {MIN_DEVICE_UNKNOWNS} the device solver's "
                             "basis holds: use engine=\"python\"")
        rc, values, Vt, res, gn, rec = device_curvature(prob, point, k, rel_tol, int(max_iters), shift, lib_path, solver_settings)
        V = np.ascontiguousarray(Vt.T)
        if rc != 0:
            bad = [j for j in range(k) if not res[j] <= rel_tol * rec["h_max"]]
            raise RuntimeError("hessian_spectrum: " + ", ".join(f"mode {j} (residual {res[j]:.3e})" for j in bad)
                               + f" did not reach {rel_tol:g} * h_max = {rel_tol * rec['h_max']:.3e} in {max_iters} iterations")
    try:
        default_variables = _select(prob, None)[0]
    except ValueError:  # (a graph without landmarks whose only chain is the fixed pose)
        default_variables = []
    curvature = Curvature(values, V, res, gn, names, first, size, rec["h_max"], rel_tol, default_variables)
    info = {"h_max": float(rec["h_max"]), "shift": float(rec["shift"]), "c_max": float(rec["c_max"]),
            "iterations": int(rec["iterations"]), "unconverged": int(rec["unconverged"]), "setup_ms": float(rec["setup_ms"]),
            "solve_ms": float(rec["solve_ms"]), "engine": engine}
    return curvature, info


def escape(data, results, curvature: Curvature, steps=(0.25, 0.5, 1.0, 2.0, 4.0), range_weights=None, loop_closure_weights=None):
    """Leave a saddle: ``results`` retracted by +t v_0 or -t v_0 (v_0: the mode of the lowest, negative value), whichever of
    the signs and of the ``steps`` t gives the lowest cost.  Returns the ``SolverResults`` there; the caller refines from it.
    ValueError where ``curvature`` has no negative mode, RuntimeError where no step lowers the cost."""
    if not curvature.negative():
        raise ValueError("escape: the curvature has no negative mode: nothing to escape from")
    prob, point = _problem_and_point(data, results, range_weights, loop_closure_weights)
    v0 = curvature.vectors[:, 0]
    if v0.shape != (prob.n,):
        raise ValueError(f"escape: the curvature's modes have {v0.shape[0]} rows, the graph {prob.n} unknowns")
    best, best_cost = None, prob.cost(point)
    for t in steps:
        for sign in (1.0, -1.0):
            trial = prob.retract(point, sign * float(t) * v0)
            f = prob.cost(trial)
            if f < best_cost:
                best, best_cost = trial, f
    if best is None:
        raise RuntimeError("escape: no step along the negative mode lowers the cost")
    return _as_results(prob, best, results, best_cost)


__all__ = ["hessian_spectrum", "escape", "dense_hessian", "sparse_hessian", "curvature_term", "Curvature", "CurvatureHandle",
           "device_curvature", "CURVATURE_SYMBOLS"]

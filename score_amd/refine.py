"""Local refinement after SCORE (reference README.md:63-67).

SCORE's convex relaxation gives an initial estimate; the reference's README hands it to a local
nonlinear least-squares solver (GTSAM in the paper) for the maximum-likelihood estimate on the
manifold.  This module is that next step, in 2-D and in 3-D: Gauss-Newton with Levenberg-Marquardt damping
on SE(d)^N x R^(d L) (3-D: steps in the tangent space, retraction R <- R Exp(omega), t <- t + v; class
``_Problem3D``), the first pose of the first chain held fixed (the gauge SCORE fixes too), over
exactly the factors SCORE reads (relative-pose measurements with the reference's chordal rotation cost,
gurobi_utils.py:504-526; ranges :449-501; landmark priors :433-446):

    F(theta, t, l) = sum_rel  kappa |t_j - t_i - R(theta_i) t_ij|^2 + tau |R(theta_j) - R(theta_i) R_ij|_F^2
                   + sum_rng  w (|p_a - p_b| - d_ab)^2  +  sum_prior w |l - l0|^2

The residuals and the sparse Jacobian are assembled vectorised on the host (NumPy / SciPy); the damped
normal equations (J'J + lambda I) step = -J'r -- block-tridiagonal 3 x 3 pose chains along every
robot's odometry, plus loop-closure and range couplings -- are solved on the GPU by the solver's
chain-preconditioned PCG through the C ABI (``score_linear_create`` / ``score_linear_solve``:
``k_factor`` factors the chains of J'J, ``k_prec_pre`` + ``k_spmv`` run the PCG, termination on the
device).  ``linear_solver="scipy"`` keeps the sparse-LU solve on the host: the reference the tests
compare the device path with, not a fallback (the default path raises without the HIP library).

``engine="native"`` (default) runs the WHOLE loop behind the C ABI (``score_refine_create`` /
``score_refine_run``, csrc/score_gn.hpp): per-measurement Jacobian blocks, J'J / J'r on a fixed pattern
and trial points are device kernels too, the host only steers the Levenberg-Marquardt iteration.
``engine="python"`` is the loop below (host Jacobians), kept as the readable twin the tests compare with.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from . import compat
from .bindings import bind, ptr
from .native import graph_arrays, score_graph_struct
from .solver import LinearSolver, ScoreRefineInfo, load_library, make_settings


def _weighted_ranges(a: dict, range_weights) -> dict:
    """The graph's arrays with every range precision scaled by its weight (``range_weights``: one per range, in the order of
    ``graph_arrays``' ``rng_*`` -- what ``solve_score_robust`` returns in ``info["robust"]["weights"]``); None: as they are."""
    if range_weights is None:
        return a
    w = np.asarray(range_weights, dtype=np.float64)
    if w.shape != (len(a["rng_a"]),):
        raise ValueError(f"range_weights: {len(a['rng_a'])} weights expected (one per range), got shape {w.shape}")
    if not (np.all(np.isfinite(w)) and np.all(w >= 0)):
        raise ValueError("range_weights must be finite and non-negative")
    out = dict(a)
    out["rng_prec"] = np.ascontiguousarray(np.asarray(a["rng_prec"], dtype=np.float64) * w)
    return out


def _weighted_loop_closures(a: dict, loop_closure_weights) -> dict:
    """The graph's arrays with kappa and tau of every loop closure (the trailing relative-pose entries) scaled by its weight
    (``loop_closure_weights``: one per loop closure, in the order of ``data.loop_closure_measurements`` -- what
    ``solve_score_robust`` returns in ``info["robust"]["loop_closure_weights"]``); None: as they are."""
    if loop_closure_weights is None:
        return a
    n_lc = int(len(a["rel_base"]) - int(np.sum(np.asarray(a["chain_len"], dtype=np.int64) - 1)))
    w = np.asarray(loop_closure_weights, dtype=np.float64)
    if w.shape != (n_lc,):
        raise ValueError(f"loop_closure_weights: {n_lc} weights expected (one per loop closure), got shape {w.shape}")
    if not (np.all(np.isfinite(w)) and np.all(w >= 0)):
        raise ValueError("loop_closure_weights must be finite and non-negative")
    out = dict(a)
    for key in ("rel_kappa", "rel_tau"):
        v = np.array(a[key], dtype=np.float64)
        v[len(v) - n_lc:] *= w
        out[key] = v
    return out


class _Problem:
    """Residuals and sparse Jacobian of the 2-D RA-SLAM least-squares problem in the minimal
    parametrisation u = [theta_1.., x_1, y_1.. | landmarks]; pose 0 (first pose of chain 0) is fixed."""

    def __init__(self, data, range_weights=None, loop_closure_weights=None):
        if data.dimension != 2:
            raise ValueError("refine_estimate: 2-D graphs only")
        a = _weighted_loop_closures(_weighted_ranges(graph_arrays(data), range_weights), loop_closure_weights)
        self.a = a
        self.Np, self.Nl = len(a["pose_names"]), len(a["landmark_names"])
        self.n = 3 * (self.Np - 1) + 2 * self.Nl
        self.bi, self.tj = a["rel_base"].astype(np.int64), a["rel_to"].astype(np.int64)
        self.tm, self.Rm = a["rel_t"], a["rel_R"]
        self.sk, self.st = np.sqrt(a["rel_kappa"]), np.sqrt(a["rel_tau"])
        self.ra, self.rb = a["rng_a"].astype(np.int64), a["rng_b"].astype(np.int64)
        self.dist, self.sw = a["rng_dist"], np.sqrt(a["rng_prec"])
        self.pl, self.pt, self.spw = a["lprior_lm"].astype(np.int64), a["lprior_t"], np.sqrt(a["lprior_prec"])
        self.pin = (0.0, np.zeros(2))

    # ---- packing ----
    def split(self, u) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        th = np.concatenate([[self.pin[0]], u[0 : 3 * (self.Np - 1) : 3]])
        t = np.vstack([self.pin[1][None, :], np.stack([u[1 : 3 * (self.Np - 1) : 3], u[2 : 3 * (self.Np - 1) : 3]], axis=1)])
        lm = u[3 * (self.Np - 1) :].reshape(-1, 2)
        return th, t, lm

    def pack(self, th, t, lm) -> np.ndarray:
        u = np.empty(self.n)
        u[0 : 3 * (self.Np - 1) : 3] = th[1:]
        u[1 : 3 * (self.Np - 1) : 3] = t[1:, 0]
        u[2 : 3 * (self.Np - 1) : 3] = t[1:, 1]
        u[3 * (self.Np - 1) :] = lm.ravel()
        return u

    def _col_pose(self, p):  # first column of pose p (theta, x, y); -1 for the fixed pose
        return np.where(p > 0, 3 * (p - 1), -1)

    def _point(self, v, t, lm):
        pose = v < self.Np
        out = np.empty((len(v), 2))
        out[pose] = t[v[pose]]
        out[~pose] = lm[v[~pose] - self.Np]
        return out

    def _col_point(self, v):  # column of x of a range endpoint
        pose = v < self.Np
        return np.where(pose, np.where(v > 0, 3 * (v - 1) + 1, -1), 3 * (self.Np - 1) + 2 * (v - self.Np))

    # ---- residuals / Jacobian ----
    def residuals(self, u, jac: bool = False):
        th, t, lm = self.split(u)
        c, s = np.cos(th), np.sin(th)
        bi, tj = self.bi, self.tj
        ne = len(bi)
        ci, si, cj, sj = c[bi], s[bi], c[tj], s[tj]
        tm, Rm = self.tm, self.Rm
        # translation: t_j - t_i - R_i tm
        rt = t[tj] - t[bi] - np.stack([ci * tm[:, 0] - si * tm[:, 1], si * tm[:, 0] + ci * tm[:, 1]], axis=1)
        # rotation (chordal): R_j - R_i Rm, the four entries
        Ri = np.stack([ci, -si, si, ci], axis=1).reshape(ne, 2, 2)
        Rj = np.stack([cj, -sj, sj, cj], axis=1).reshape(ne, 2, 2)
        rr = (Rj - Ri @ Rm).reshape(ne, 4)
        pa, pb = self._point(self.ra, t, lm), self._point(self.rb, t, lm)
        dv = pa - pb
        rho = np.sqrt(np.einsum("ij,ij->i", dv, dv))
        rg = rho - self.dist
        rp = lm[self.pl] - self.pt if len(self.pl) else np.zeros((0, 2))
        res = np.concatenate([(self.sk[:, None] * rt).ravel(), (self.st[:, None] * rr).ravel(), self.sw * rg,
                              (self.spw[:, None] * rp).ravel()])
        if not jac:
            return res
        rows, cols, vals = [], [], []

        def add(r, cidx, v):
            keep = cidx >= 0
            rows.append(r[keep]); cols.append(cidx[keep]); vals.append(v[keep])

        e = np.arange(ne)
        coli, colj = self._col_pose(bi), self._col_pose(tj)
        # translation rows 2e, 2e+1
        for k in range(2):
            r = 2 * e + k
            add(r, np.where(colj >= 0, colj + 1 + k, -1), self.sk)
            add(r, np.where(coli >= 0, coli + 1 + k, -1), -self.sk)
        dRt = np.stack([-si * tm[:, 0] - ci * tm[:, 1], ci * tm[:, 0] - si * tm[:, 1]], axis=1)  # d(R_i tm)/dtheta_i
        for k in range(2):
            add(2 * e + k, coli, -self.sk * dRt[:, k])
        # rotation rows
        base = 2 * ne
        dRi = np.stack([-si, -ci, ci, -si], axis=1).reshape(ne, 2, 2)
        dRj = np.stack([-sj, -cj, cj, -sj], axis=1).reshape(ne, 2, 2)
        dri = -(dRi @ Rm).reshape(ne, 4)
        drj = dRj.reshape(ne, 4)
        for k in range(4):
            add(base + 4 * e + k, coli, self.st * dri[:, k])
            add(base + 4 * e + k, colj, self.st * drj[:, k])
        # ranges
        base += 4 * ne
        nr = len(self.ra)
        r = base + np.arange(nr)
        safe = np.where(rho > 1e-12, rho, 1.0)
        g = dv / safe[:, None]
        g[rho <= 1e-12] = 0.0
        ca, cb = self._col_point(self.ra), self._col_point(self.rb)
        for k in range(2):
            add(r, np.where(ca >= 0, ca + k, -1), self.sw * g[:, k])
            add(r, np.where(cb >= 0, cb + k, -1), -self.sw * g[:, k])
        base += nr
        npz = len(self.pl)
        for k in range(2):
            add(base + 2 * np.arange(npz) + k, 3 * (self.Np - 1) + 2 * self.pl + k, self.spw)
        J = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(len(res), self.n))
        return res, J

    def cost(self, u) -> float:
        r = self.residuals(u)
        return float(r @ r)

    def retract(self, u, step):
        return u + step

    def chains(self):
        """One 3 x 3 chain per robot, node = pose (theta, x, y); the pinned pose is not an unknown."""
        lens = np.asarray(self.a["chain_len"], dtype=np.int64).copy()
        lens[0] -= 1
        lens = lens[lens > 0]
        return np.concatenate([[0], np.cumsum(lens)]), 3 * np.arange(self.Np - 1, dtype=np.int64)


def _hat(v: np.ndarray) -> np.ndarray:
    """[v]x for a stack of 3-vectors."""
    K = np.zeros(v.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -v[..., 2], v[..., 1]
    K[..., 1, 0], K[..., 1, 2] = v[..., 2], -v[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -v[..., 1], v[..., 0]
    return K


def so3_exp(w: np.ndarray) -> np.ndarray:
    """Rodrigues' formula for a stack of rotation vectors."""
    th = np.linalg.norm(w, axis=-1)
    K = _hat(w)
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    A = np.where(small, 1.0 - th ** 2 / 6.0, np.sin(ths) / ths)
    B = np.where(small, 0.5 - th ** 2 / 24.0, (1.0 - np.cos(ths)) / ths ** 2)
    return np.eye(3) + A[..., None, None] * K + B[..., None, None] * (K @ K)


class _Problem3D:
    """The 3-D RA-SLAM least-squares problem on SE(3)^N x R^(3 L) (the reference's model is dimension-generic,
    gurobi_utils.py:37-50).  The STATE is (R, t, lm): rotation matrices, translations, landmarks; a STEP lives in the
    tangent space, (omega, v) per free pose and a 3-vector per landmark, applied by the retraction
    R <- R Exp(omega), t <- t + v.  Columns of pose p >= 1: 6 (p - 1) .. +5 = [omega | v]; pose 0 is fixed."""

    def __init__(self, data, range_weights=None, loop_closure_weights=None):
        if data.dimension != 3:
            raise ValueError("_Problem3D: 3-D graphs only")
        a = _weighted_loop_closures(_weighted_ranges(graph_arrays(data), range_weights), loop_closure_weights)
        self.a = a
        self.Np, self.Nl = len(a["pose_names"]), len(a["landmark_names"])
        self.n = 6 * (self.Np - 1) + 3 * self.Nl
        self.bi, self.tj = a["rel_base"].astype(np.int64), a["rel_to"].astype(np.int64)
        self.tm, self.Rm = a["rel_t"], a["rel_R"]
        self.sk, self.st = np.sqrt(a["rel_kappa"]), np.sqrt(a["rel_tau"])
        self.ra, self.rb = a["rng_a"].astype(np.int64), a["rng_b"].astype(np.int64)
        self.dist, self.sw = a["rng_dist"], np.sqrt(a["rng_prec"])
        self.pl, self.pt, self.spw = a["lprior_lm"].astype(np.int64), a["lprior_t"].reshape(-1, 3), np.sqrt(a["lprior_prec"])

    def _point(self, v, t, lm):
        pose = v < self.Np
        out = np.empty((len(v), 3))
        out[pose] = t[v[pose]]
        out[~pose] = lm[v[~pose] - self.Np]
        return out

    def retract(self, state, step):
        R, t, lm = state
        w = step[: 6 * (self.Np - 1)].reshape(-1, 6)
        Rn, tn = R.copy(), t.copy()
        Rn[1:] = R[1:] @ so3_exp(w[:, :3])
        tn[1:] = t[1:] + w[:, 3:]
        return Rn, tn, lm + step[6 * (self.Np - 1):].reshape(-1, 3)

    def residuals(self, state, jac: bool = False):
        R, t, lm = state
        bi, tj = self.bi, self.tj
        ne = len(bi)
        rt = t[tj] - t[bi] - np.einsum("eij,ej->ei", R[bi], self.tm)
        rR = (R[tj] - R[bi] @ self.Rm).reshape(ne, 9)
        pa, pb = self._point(self.ra, t, lm), self._point(self.rb, t, lm)
        dv = pa - pb
        rho = np.linalg.norm(dv, axis=1)
        rp = lm[self.pl] - self.pt if len(self.pl) else np.zeros((0, 3))
        res = np.concatenate([(self.sk[:, None] * rt).ravel(), (self.st[:, None] * rR).ravel(), self.sw * (rho - self.dist),
                              (self.spw[:, None] * rp).ravel()])
        if not jac:
            return res
        rows, cols, vals = [], [], []

        def add(r, c, v):
            r, c, v = np.broadcast_arrays(np.asarray(r), np.asarray(c), np.asarray(v))
            r, c, v = r.ravel(), c.ravel(), v.ravel()
            keep = c >= 0
            rows.append(r[keep]); cols.append(c[keep]); vals.append(v[keep])

        NEG = -(10 ** 9)
        e = np.arange(ne)
        ci, cj = np.where(bi > 0, 6 * (bi - 1), NEG), np.where(tj > 0, 6 * (tj - 1), NEG)
        k3 = np.arange(3)
        r_t = 3 * e[:, None] + k3[None, :]
        add(r_t, cj[:, None] + 3 + k3[None, :], self.sk[:, None])
        add(r_t, ci[:, None] + 3 + k3[None, :], -self.sk[:, None])
        M = R[bi] @ _hat(self.tm)  # d r_t / d omega_i = R_i [tm]x
        for a_ in range(3):
            add(r_t, ci[:, None] + a_, self.sk[:, None] * M[:, :, a_])
        base = 3 * ne
        r_R = base + 9 * e[:, None] + np.arange(9)[None, :]
        for a_ in range(3):
            Ea = _hat(np.eye(3)[a_])
            add(r_R, cj[:, None] + a_, self.st[:, None] * (R[tj] @ Ea).reshape(ne, 9))
            add(r_R, ci[:, None] + a_, -self.st[:, None] * (R[bi] @ Ea @ self.Rm).reshape(ne, 9))
        base += 9 * ne
        nr = len(self.ra)
        r = base + np.arange(nr)
        g = dv / np.where(rho > 1e-12, rho, 1.0)[:, None]
        g[rho <= 1e-12] = 0.0

        def pcol(v):
            pose = v < self.Np
            return np.where(pose, np.where(v > 0, 6 * (v - 1) + 3, NEG), 6 * (self.Np - 1) + 3 * (v - self.Np))

        add(r[:, None], pcol(self.ra)[:, None] + k3[None, :], self.sw[:, None] * g)
        add(r[:, None], pcol(self.rb)[:, None] + k3[None, :], -self.sw[:, None] * g)
        base += nr
        npz = len(self.pl)
        add(base + 3 * np.arange(npz)[:, None] + k3[None, :], 6 * (self.Np - 1) + 3 * self.pl[:, None] + k3[None, :], self.spw[:, None])
        J = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(len(res), self.n))
        return res, J

    def cost(self, state) -> float:
        r = self.residuals(state)
        return float(r @ r)

    def initial_state(self, results):
        T = _stacked(results.poses, self.a["pose_names"], (4, 4))
        lm = _stacked(results.landmarks, self.a["landmark_names"], (3,)) if self.Nl else np.zeros((0, 3))
        return T[:, :3, :3].copy(), T[:, :3, 3].copy(), lm.copy()

    def chains(self):
        """3 x 3 chains of the preconditioner: per robot the omega blocks and the v blocks of its free poses."""
        lens = np.asarray(self.a["chain_len"], dtype=np.int64)
        ptr, first, p0 = [0], [], 0
        for L in lens:
            ps = np.arange(p0, p0 + L)
            ps = ps[ps > 0]
            for kind in range(2):
                if ps.size:
                    first.append(6 * (ps - 1) + 3 * kind)
                    ptr.append(ptr[-1] + ps.size)
            p0 += L
        return np.asarray(ptr, dtype=np.int64), (np.concatenate(first) if first else np.zeros(0, np.int64))


def _stacked(mapping, names, shape):
    """Values of ``mapping`` in the order of ``names`` as one array: without a Python loop when the mapping is
    an ArrayDict over the same names (what solve_score returns)."""
    if isinstance(mapping, compat.ArrayDict) and len(mapping) == len(names) and list(mapping.keys()) == list(names):
        return np.asarray(mapping.array, dtype=np.float64).reshape((len(names),) + shape)
    return np.array([np.asarray(mapping[nm], dtype=np.float64) for nm in names], dtype=np.float64).reshape((len(names),) + shape)


def _initial_point(prob: _Problem, results) -> np.ndarray:
    T = _stacked(results.poses, prob.a["pose_names"], (3, 3))
    th = np.arctan2(T[:, 1, 0], T[:, 0, 0])
    t = T[:, :2, 2].copy()
    lm = _stacked(results.landmarks, prob.a["landmark_names"], (2,))
    prob.pin = (float(th[0]), t[0].copy())
    return prob.pack(th, t, lm)


class _DeviceNormalEquations:
    """(J'J + lambda I) step = rhs on the GPU.  The pattern of J'J is fixed by the graph: it is taken once
    from the all-ones Jacobian (no cancellation can remove an entry), a linear-mode handle is created on it
    with one chain per robot (node = pose: theta, x, y), and every solve maps the current values onto it."""

    def __init__(self, prob: _Problem, J: sp.csr_matrix, lib_path: Optional[str], settings: Optional[dict]):
        ones = J.copy()
        ones.data[:] = 1.0
        pat = (ones.T @ ones + sp.identity(prob.n, format="csr")).tocsr()
        pat.sort_indices()
        self.n = prob.n
        self.indptr, self.indices = pat.indptr.astype(np.int64), pat.indices.astype(np.int64)
        rows = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.indptr))
        self.keys = rows * self.n + self.indices  # ascending: CSR with sorted indices
        self.diag = np.searchsorted(self.keys, np.arange(self.n, dtype=np.int64) * (self.n + 1))
        chain_ptr, node_first_col = prob.chains()
        self.solver = LinearSolver(pat, chain_ptr, node_first_col, 3, settings=settings, lib_path=lib_path)
        self._cache = None  # (indptr, indices) of the last J'J and its positions in the pattern
        self.pcg_iters = 0
        self.solves = 0

    def values(self, H: sp.csr_matrix) -> np.ndarray:
        c = self._cache
        if c is None or c[0].shape != H.indptr.shape or c[1].shape != H.indices.shape or \
                not (np.array_equal(c[0], H.indptr) and np.array_equal(c[1], H.indices)):
            rows = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(H.indptr))
            pos = np.searchsorted(self.keys, rows * self.n + H.indices.astype(np.int64))
            if pos.size and (pos.max() >= self.keys.size or not np.array_equal(self.keys[pos], rows * self.n + H.indices)):
                raise RuntimeError("refine: J'J left its sparsity pattern")
            self._cache = c = (H.indptr.copy(), H.indices.copy(), pos)
        v = np.zeros(self.keys.size)
        if H.has_canonical_format:
            v[c[2]] = H.data
        else:
            np.add.at(v, c[2], H.data)  # duplicates summed
        return v

    def solve(self, H: sp.csr_matrix, lam: float, rhs: np.ndarray, rel_tol: float) -> np.ndarray:
        v = self.values(H)
        v[self.diag] += lam
        x, info = self.solver.solve(v, rhs, rel_tol=rel_tol, max_iters=4000)
        self.pcg_iters += info["iters"]
        self.solves += 1
        if not np.all(np.isfinite(x)):
            raise RuntimeError("refine: the device PCG returned a non-finite step")
        return x

    def close(self) -> None:
        self.solver.close()


class _Handle:
    """A handle of the library with the context manager that destroys it.  ``headers``: the tables (``bindings.Table``) of the
    calls the handle makes; subclasses extend them.  They are bound before the handle is created, so a library that lacks a
    symbol is refused with nothing to release."""

    headers: tuple = ()
    destroy = "score_refine_destroy"

    def __init__(self, lib_path: Optional[str], solver_settings: Optional[dict]):
        self.lib = load_library(lib_path)
        for table in self.headers:
            bind(self.lib, table)
        self.h = C.c_void_p()
        self._create(make_settings(self.lib, solver_settings))

    def close(self) -> None:
        if self.h:
            getattr(self.lib, self.destroy)(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class RefineHandle(_Handle):
    """A refinement handle (``score_refine_create``) on one graph: points go in and come out in the problem's own form
    (``_Problem``: packed unknowns; ``_Problem3D``: (R, t, lm))."""

    def __init__(self, prob, lib_path: Optional[str] = None, solver_settings: Optional[dict] = None):
        self.prob = prob
        super().__init__(lib_path, solver_settings)

    def _create(self, st) -> None:
        g = score_graph_struct(self.prob.a)
        if self.lib.score_refine_create(C.byref(g), C.byref(st), C.byref(self.h)) != 0:
            raise RuntimeError(f"score_refine_create failed: {self.lib.score_last_error().decode()}")

    def run(self, point, max_iters: int = 50, tol: float = 1e-10):
        """``score_refine_run`` (the whole LM loop behind the C ABI): (point, info dict)."""
        poses_in, lms_in = _point_arrays(self.prob, point)
        poses_out, lms_out = _point_outputs(poses_in, lms_in)
        info = ScoreRefineInfo()
        rc = self.lib.score_refine_run(self.h, ptr(poses_in), ptr(lms_in), int(max_iters), float(tol), ptr(poses_out), ptr(lms_out),
                                       C.byref(info))
        if rc != 0:
            raise RuntimeError(f"score_refine_run failed: {self.lib.score_last_error().decode()}")
        return _point_from(self.prob, poses_out, lms_out), info.as_dict()


def _problem_and_point(data, results, range_weights=None, loop_closure_weights=None):
    """The least-squares problem of ``data`` under the weights and ``results`` as a point of it."""
    if data.dimension == 3:
        prob = _Problem3D(data, range_weights, loop_closure_weights)
        return prob, prob.initial_state(results)
    prob = _Problem(data, range_weights, loop_closure_weights)
    return prob, _initial_point(prob, results)


def _refine_native(prob: _Problem, u0: np.ndarray, max_iters: int, tol: float, lib_path: Optional[str],
                   solver_settings: Optional[dict]):
    """One ``RefineHandle.run`` on a handle of its own.  Returns (u, info dict)."""
    with RefineHandle(prob, lib_path, solver_settings) as h:
        return h.run(u0, max_iters, tol)


def _native_info(ni: dict, iterations: str = "iterations") -> dict:
    """``info`` as the refinement entry points report it, from a native info record (``iterations``: the record's field)."""
    return {"cost_initial": ni["cost_initial"], "cost_final": ni["cost_final"], "iterations": ni[iterations],
            "grad_inf": ni["grad_inf"], "linear_solver": "device", "engine": "native", "pcg_iters": ni["pcg_iters"],
            "linear_solves": ni["linear_solves"], "setup_ms": ni["setup_ms"], "solve_ms": ni["solve_ms"]}


def refine_estimate(data, results, max_iters: int = 50, tol: float = 1e-10, verbose: bool = False,
                    linear_solver: str = "device", lib_path: Optional[str] = None, solver_settings: Optional[dict] = None,
                    pcg_rel_tol: float = 1e-9, engine: str = "native", range_weights=None,
                    loop_closure_weights=None):
    """Refine a SCORE estimate (``SolverResults``) to a local minimiser of the RA-SLAM maximum-likelihood
    cost.  Returns ``(refined SolverResults, info)``; ``info`` holds the cost before / after, iterations,
    the final gradient norm and (device path) the PCG iterations spent in the linear solves.
    ``range_weights`` (one per range, in the graph's range order): the range precisions are scaled by them -- the weights of
    ``solve_score_robust`` (``info["robust"]["weights"]``) keep the ranges it flagged out of the maximum-likelihood step.
    ``loop_closure_weights`` (one per loop closure, in the order of ``data.loop_closure_measurements``) scale kappa and tau of
    the loop closures in the same way (``info["robust"]["loop_closure_weights"]``)."""
    if linear_solver not in ("device", "scipy"):
        raise ValueError("linear_solver must be 'device' or 'scipy'")
    if engine not in ("native", "python"):
        raise ValueError("engine must be 'native' or 'python'")
    prob, u = _problem_and_point(data, results, range_weights, loop_closure_weights)
    if engine == "native" and linear_solver == "device" and prob.n > 0:
        u, ni = _refine_native(prob, u, max_iters, tol, lib_path, solver_settings)
        return _as_results(prob, u, results, ni["cost_final"]), _native_info(ni)
    res, J = prob.residuals(u, jac=True)
    dev = _DeviceNormalEquations(prob, J, lib_path, solver_settings) if (linear_solver == "device" and prob.n > 0) else None
    try:
        u, m = _lm_loop(prob, u, res, J, float(res @ res), max_iters, tol, verbose, dev, pcg_rel_tol)
    finally:
        pcg = (dev.pcg_iters, dev.solves) if dev else (0, 0)
        if dev:
            dev.close()
    info = {"cost_initial": m.cost_initial, "cost_final": m.f, "iterations": m.iterations, "grad_inf": m.gnorm,
            "linear_solver": linear_solver, "engine": "python", "pcg_iters": pcg[0], "linear_solves": pcg[1]}
    return _as_results(prob, u, results, m.f), info


def _as_results(prob, u, results, cost: float):
    if isinstance(prob, _Problem3D):
        R, t, lm = u
        T = np.tile(np.eye(4), (prob.Np, 1, 1))
        T[:, :3, :3] = R
        T[:, :3, 3] = t
        values = compat.VariableValues(3, compat.ArrayDict(prob.a["pose_names"], T), compat.ArrayDict(prob.a["landmark_names"], np.array(lm, dtype=np.float64)), None)
        return compat.SolverResults(variables=values, total_time=results.total_time, solved=True,
                                    pose_chain_names=results.pose_chain_names, solver_cost=cost, info=dict(results.info or {}))
    th, t, lm = prob.split(u)
    c, s = np.cos(th), np.sin(th)
    T = np.tile(np.eye(3), (prob.Np, 1, 1))
    T[:, 0, 0] = c; T[:, 0, 1] = -s; T[:, 1, 0] = s; T[:, 1, 1] = c
    T[:, :2, 2] = t
    values = compat.VariableValues(2, compat.ArrayDict(prob.a["pose_names"], T), compat.ArrayDict(prob.a["landmark_names"], lm.copy()), None)
    return compat.SolverResults(variables=values, total_time=results.total_time, solved=True,
                                pose_chain_names=results.pose_chain_names, solver_cost=cost, info=dict(results.info or {}))


# ---------------------------------------------------------------------------------------------------------------------
# the point in the C ABI's layout
# ---------------------------------------------------------------------------------------------------------------------
def _point_arrays(prob, point):
    if isinstance(prob, _Problem3D):  # [R (row-major) | t] per pose, landmarks x 3
        R, t, lm = point
        poses = np.ascontiguousarray(np.concatenate([R.reshape(prob.Np, 9), t], axis=1), dtype=np.float64)
        return poses, np.ascontiguousarray(lm, dtype=np.float64).reshape(-1, 3)
    th, t, lm = prob.split(point)
    return np.ascontiguousarray(np.column_stack([th, t]), dtype=np.float64), np.ascontiguousarray(lm, dtype=np.float64).reshape(-1, 2)


def _point_outputs(poses_in, lms_in):
    """Arrays for the point a call writes (the landmarks' is never empty)."""
    return np.empty_like(poses_in), np.empty((max(1, len(lms_in)), lms_in.shape[1]))


def _point_from(prob, poses, lms):
    if isinstance(prob, _Problem3D):
        return poses[:, :9].reshape(-1, 3, 3).copy(), poses[:, 9:12].copy(), lms[: prob.Nl].copy()
    return prob.pack(poses[:, 0], poses[:, 1:3], lms[: prob.Nl])


def unknown_sizes(prob) -> Tuple[int, int]:
    """(d, dp): the unknowns of a landmark and of a pose -- (2, 3) for (theta, x, y), (3, 6) for (omega, v)."""
    return (3, 6) if isinstance(prob, _Problem3D) else (2, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the Levenberg-Marquardt step rule (the library's is csrc/score_refine_rule.hpp: LmState and lm_*), and its drivers: _lm_loop
# here, refine_batch._LockStep for a group
# ---------------------------------------------------------------------------------------------------------------------
GRADIENT, SOLVE, STOPPED = "gradient", "solve", "stopped"


class _Member:
    """The state of one Levenberg-Marquardt run, and its transitions (pure: they read and write this record only)."""

    def __init__(self, f: float, max_iters: int):
        self.f = self.cost_initial = float(f)
        self.lam, self.gnorm = 1e-6, float("inf")
        self.it, self.attempts, self.iterations, self.linear_solves, self.pcg_iters = 1, 0, 0, 0, 0
        self.phase = GRADIENT
        if self.it > max_iters:
            self._stop(max_iters)

    def _stop(self, max_iters: int) -> None:
        self.phase = STOPPED
        self.iterations = min(self.it, max_iters)

    def after_gradient(self, gnorm: float, tol: float, max_iters: int) -> None:
        """Top of iteration ``it``: the gradient of the current point is known."""
        self.gnorm = float(gnorm)
        if gnorm <= tol * max(1.0, self.f):
            self._stop(max_iters)
            return
        self.attempts = 0
        self.phase = SOLVE

    def after_solve(self, ok: bool, used: int, fn: float, max_iters: int) -> bool:
        """One attempt: the solve and, where it succeeded, the cost at the trial point.  True: the step is accepted."""
        self.linear_solves += 1
        self.pcg_iters += int(used)
        if ok and fn < self.f:
            dec = self.f - fn
            self.f = float(fn)
            self.lam = max(self.lam * 0.1, 1e-12)
            if dec <= 1e-14 * max(1.0, self.f):
                self._stop(max_iters)
                return True
            self.it += 1
            if self.it > max_iters:
                self._stop(max_iters)
            else:
                self.phase = GRADIENT
            return True
        self.lam *= 10.0
        self.attempts += 1
        if self.attempts >= 12:
            self._stop(max_iters)
        return False


def _gradient(res, J):
    """g = J'r and |g|_inf."""
    g = J.T @ res
    return g, float(np.abs(g).max()) if g.size else 0.0


def _attempt(prob, u, H, g, lam: float, dev=None, pcg_rel_tol: float = 1e-9):
    """One damped solve, trial point and cost: (solved, trial point, its cost)."""
    try:
        if dev:
            step = dev.solve(H, lam, -g, pcg_rel_tol)
        else:
            step = spla.splu((H + lam * sp.identity(prob.n, format="csc")).tocsc()).solve(-g)
    except RuntimeError:
        return False, None, float("nan")
    un = prob.retract(u, step)
    return True, un, prob.cost(un)


def _lm_loop(prob, u, res, J, f, max_iters, tol, verbose, dev, pcg_rel_tol):
    """One run from ``u`` (``res``, ``J``, ``f``: residuals, Jacobian and cost there): (the point it ends at, its ``_Member``).
    The residuals and the Jacobian of an accepted point are evaluated only when another iteration follows."""
    m = _Member(f, max_iters)
    while m.phase == GRADIENT:
        g, gnorm = _gradient(res, J)
        m.after_gradient(gnorm, tol, max_iters)
        if m.phase != SOLVE:
            break
        H = (J.T @ J).tocsr() if dev else (J.T @ J).tocsc()
        it, accepted = m.it, False
        while m.phase == SOLVE and not accepted:
            ok, un, fn = _attempt(prob, u, H, g, m.lam, dev, pcg_rel_tol)
            accepted = m.after_solve(ok, 0, fn, max_iters)
        if not accepted:
            break
        u = un
        if m.phase == GRADIENT:
            res, J = prob.residuals(u, jac=True)
        if verbose:
            print(f"  refine it {it}: cost {m.f:.9g} |g| {m.gnorm:.3e} lambda {m.lam:.1e}")
    return u, m

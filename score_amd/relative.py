"""Predicted relative poses between pairs of poses and their covariances at a refined estimate (include/score_relative.h):
the Mahalanobis gate in front of a loop closure.

Marginals and samples say how uncertain a variable is, ``predicted_range_variances`` what a hypothetical range is worth.
Before a place-recognition match enters the graph the question is another one: the estimate says pose a and pose b are
T_a^-1 T_b apart, give or take P -- is the match compatible with that, and what would it add?  For a pair (a, b) of poses

    R_ab = R_a' R_b,    t_ab = R_a' (t_b - t_a),    P = G H^-1 G',

with H = J'J at the estimate and G (DP x 2 DP; DP = 3 in 2-D, 6 in 3-D) the derivative of the error coordinates xi of the
relative pose -- rotation first: 2-D (theta_ab + xi_0, t_ab + xi_1:2), 3-D (R_ab Exp(xi_0:2), t_ab + xi_3:5) -- in the
unknowns of a and b ((theta, x, y), or (omega, v) of the retraction R Exp(omega), t + v; the fixed first pose has none).
``predicted_relative_poses`` solves the DP columns H x = G'e_q of a pair on the device (``score_refine_relative_covariances``,
the marginals' block PCG) where the joint marginal of both ends takes 2 DP and leaves G to the caller; ``engine="python"``
restates it in NumPy with the dense H: small graphs, the tests, the CPU twin.

Noise of a measured relative pose.  The refinement's cost of a relative pose is kappa |t_j - t_i - R_i t_m|^2
+ tau |R_j - R_i R_m|_F^2 (csrc/score_gn.hpp, ``gn_rel_jac``: sqrt(kappa) weighs the translation rows, sqrt(tau) the rotation
rows).  To first order |R_j - R_i R_m|_F^2 = 2 |xi_rot|^2, so a measurement with ``translation_precision`` = kappa and
``rotation_precision`` = tau has the noise N = diag(I / (2 tau), I / kappa) in the error coordinates (rotation first) --
the names are those of the loop closures' attributes.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import RELATIVE, ScoreMarginalsInfo, bind, ptr, steps_and_converged
from .leverage import LeverageHandle, _singular, pair_ids
from .marginals import MAX_BLOCK_WIDTH, _problem_and_point, check_block_solve, dense_information
from .refine import _hat, _point_arrays, _Problem3D, unknown_sizes
from .solver import _i32p, load_library

# the symbols include/score_relative.h declares
RELATIVE_SYMBOLS = list(RELATIVE)


def _bind(lib: C.CDLL) -> C.CDLL:
    return bind(lib, RELATIVE)


class RelativeHandle(LeverageHandle):
    """A refinement handle kept for ``score_refine_relative_covariances`` calls on one graph (and, being a ``LeverageHandle``,
    for the leverages, the range variances and the draws)."""

    headers = LeverageHandle.headers + (RELATIVE,)

    def relative_covariances(self, point, pair_ids, rel_tol=1e-10, max_iters=4000, block_width=MAX_BLOCK_WIDTH,
                             with_solutions=False) -> dict:
        """``score_refine_relative_covariances`` as it is.  ``pair_ids``: (C, 2) pose ids.  Returns a dict: ``rc``,
        ``rotations`` (C x d x d), ``translations`` (C x d), ``covariances`` (C x dp x dp, column q as computed),
        ``residuals``, ``iterations``, ``converged`` (C x dp), ``solutions`` (asked for: C dp x n, x_j as computed; else
        None) and ``info``."""
        d, dp = unknown_sizes(self.prob)
        poses, lms = _point_arrays(self.prob, point)
        pairs = np.asarray(pair_ids, dtype=np.int32).reshape(-1, 2)
        pa, pb = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        n = len(pa)
        rot, trans, cov = np.zeros((n, d, d)), np.zeros((n, d)), np.zeros((n, dp, dp))
        res, its = np.zeros((n, dp)), np.zeros((n, dp), dtype=np.int32)
        sol = np.zeros((n * dp, self.prob.n)) if with_solutions else None
        info = ScoreMarginalsInfo()
        rc = self.lib.score_refine_relative_covariances(self.h, ptr(poses), ptr(lms), ptr(pa, _i32p), ptr(pb, _i32p), n,
                                                        float(rel_tol), int(max_iters), int(block_width), ptr(rot), ptr(trans),
                                                        ptr(cov), ptr(res), ptr(its, _i32p), ptr(sol), C.byref(info))
        if rc < 0:
            raise RuntimeError(f"score_refine_relative_covariances failed: {self.lib.score_last_error().decode()}")
        iterations, converged = steps_and_converged(its)
        return {"rc": rc, "rotations": rot, "translations": trans, "covariances": cov, "residuals": res, "iterations": iterations,
                "converged": converged, "solutions": sol, "info": info.as_dict()}


def _rotations_and_translations(prob, point):
    """(R (Np x d x d), t (Np x d)) of every pose at the point."""
    if isinstance(prob, _Problem3D):
        return np.asarray(point[0], dtype=np.float64), np.asarray(point[1], dtype=np.float64)
    th, t, _ = prob.split(point)
    c, s = np.cos(th), np.sin(th)
    return np.stack([c, -s, s, c], axis=1).reshape(-1, 2, 2), t


def pair_jacobian(Ra, ta, Rb, tb):
    """(G (dp x 2 dp), R_ab, t_ab) of one pair from the rotations and translations of its ends: the derivative of the error
    coordinates of T_a^-1 T_b in [unknowns of a | unknowns of b] (the module's docstring; include/score_relative.h)."""
    d = len(ta)
    dp = 3 if d == 2 else 6
    ro = dp - d
    Rab, tab = Ra.T @ Rb, Ra.T @ (tb - ta)
    G = np.zeros((dp, 2 * dp))
    if d == 2:
        G[0, 0], G[0, dp] = -1.0, 1.0
        G[1, 0], G[2, 0] = tab[1], -tab[0]  # -S t_ab
    else:
        G[:3, :3] = -Rab.T
        G[:3, dp:dp + 3] = np.eye(3)
        G[3:, :3] = _hat(tab)
    G[ro:, ro:dp] = -Ra.T
    G[ro:, dp + ro:] = Ra.T
    return G, Rab, tab


def relative_jacobians(prob, point, ids):
    """(G, R_ab, t_ab) for the pairs ``ids`` (C x 2 pose ids): G (n x C dp) dense, its column c dp + q the gradient of error
    coordinate q of pair c in the refinement's unknowns (the fixed first pose has none: its columns of the pair's Jacobian
    are left out), R_ab (C x d x d), t_ab (C x d)."""
    d, dp = unknown_sizes(prob)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1, 2)
    if len(ids) and (ids.min() < 0 or ids.max() >= prob.Np):
        raise ValueError("relative_jacobians: a pair's pose is out of range (a landmark has no relative pose)")
    if np.any(ids[:, 0] == ids[:, 1]):
        raise ValueError("relative_jacobians: a pair joins a pose to itself")
    R, t = _rotations_and_translations(prob, point)
    G = np.zeros((prob.n, len(ids) * dp))
    Rab, tab = np.zeros((len(ids), d, d)), np.zeros((len(ids), d))
    for c, (a, b) in enumerate(ids):
        g, Rab[c], tab[c] = pair_jacobian(R[a], t[a], R[b], t[b])
        for v, first in ((a, 0), (b, dp)):
            if v >= 1:
                G[dp * (v - 1):dp * v, c * dp:(c + 1) * dp] = g[:, first:first + dp].T
    return G, Rab, tab


def wrap_angle(x):
    """x wrapped to (-pi, pi]."""
    return -((-np.asarray(x, dtype=np.float64) + np.pi) % (2.0 * np.pi) - np.pi)


def so3_log(R):
    """The rotation vectors of a stack of rotation matrices (angles below pi)."""
    R = np.asarray(R, dtype=np.float64)
    w = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], axis=-1)
    s = np.linalg.norm(w, axis=-1)
    c = 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0)
    th = np.arctan2(s, c)
    small = s < 1e-8
    scale = np.where(small, 1.0 + th ** 2 / 6.0, th / np.where(small, 1.0, s))
    return w * scale[..., None]


def measurement_noise(d, translation_precision, rotation_precision, count):
    """N (count x dp x dp) = diag(I / (2 tau), I / kappa), rotation first: the noise the refinement's cost of a relative pose
    implies, kappa the translation precision and tau the rotation precision (scalars or one per pair)."""
    dp = 3 if d == 2 else 6
    kappa = np.broadcast_to(np.asarray(translation_precision, dtype=np.float64), (count,))
    tau = np.broadcast_to(np.asarray(rotation_precision, dtype=np.float64), (count,))
    if np.any(kappa <= 0) or np.any(tau <= 0):
        raise ValueError("the precisions of a relative pose must be positive")
    N = np.zeros((count, dp, dp))
    k = np.arange(dp)
    N[:, k, k] = np.where(k[None, :] < dp - d, 1.0 / (2.0 * tau[:, None]), 1.0 / kappa[:, None])
    return N


class PredictedRelativePoses:
    """Predicted relative poses T_a^-1 T_b of ``pairs`` at the estimate: ``rotation`` (C x d x d), ``translation`` (C x d),
    ``angle`` (C, 2-D only: theta_b - theta_a in (-pi, pi]; None in 3-D) and ``covariance`` (C x dp x dp, symmetric, in the
    error coordinates of the module's docstring: rotation first)."""

    def __init__(self, pairs, rotation, translation, covariance):
        self.pairs = list(pairs)
        self.rotation = np.asarray(rotation, dtype=np.float64)
        self.translation = np.asarray(translation, dtype=np.float64)
        self.covariance = np.asarray(covariance, dtype=np.float64)
        self.dimension = self.translation.shape[1]
        self.dof = 3 if self.dimension == 2 else 6
        self.angle = np.arctan2(self.rotation[:, 1, 0], self.rotation[:, 0, 0]) if self.dimension == 2 else None

    def _measured(self, measurements):
        d = self.dimension
        if len(measurements) != len(self.pairs):
            raise ValueError(f"{len(self.pairs)} pairs, {len(measurements)} measurements")
        Rm, tm = np.zeros((len(self.pairs), d, d)), np.zeros((len(self.pairs), d))
        for c, m in enumerate(measurements):
            if isinstance(m, tuple):
                Rm[c], tm[c] = np.asarray(m[0], dtype=np.float64), np.asarray(m[1], dtype=np.float64)
            else:
                Rm[c], tm[c] = np.asarray(m.rotation_matrix, dtype=np.float64), np.asarray(m.translation_vector, dtype=np.float64)
        return Rm, tm

    def innovation(self, measurements):
        """e (C x dp) of measured relative poses -- objects with the loop closures' ``rotation_matrix`` /
        ``translation_vector``, or ``(R_m, t_m)`` tuples -- in the error coordinates: 2-D (wrap(theta_m - theta_ab),
        t_m - t_ab), 3-D (Log(R_ab' R_m), t_m - t_ab)."""
        Rm, tm = self._measured(measurements)
        if self.dimension == 2:
            rot = wrap_angle(np.arctan2(Rm[:, 1, 0], Rm[:, 0, 0]) - self.angle)[:, None]
        else:
            rot = so3_log(np.einsum("cki,ckj->cij", self.rotation, Rm))
        return np.concatenate([rot, tm - self.translation], axis=1)

    def gate(self, measurements, translation_precision, rotation_precision):
        """(d2, dof): d2 (C) = e'(P + N)^-1 e for the innovation e of ``measurements`` with N = diag(I / (2 tau), I / kappa),
        kappa = ``translation_precision``, tau = ``rotation_precision`` (the loop closures' attributes; scalars or one per
        pair) -- chi^2(dof) for a match that fits the estimate, dof = 3 or 6."""
        e = self.innovation(measurements)
        S = self.covariance + measurement_noise(self.dimension, translation_precision, rotation_precision, len(self.pairs))
        return np.einsum("ci,ci->c", e, np.linalg.solve(S, e[:, :, None])[:, :, 0]), self.dof

    def information_gain(self, translation_precision, rotation_precision):
        """1/2 log det(I + N^-1 P) per pair, in nats: what a relative pose of those precisions would add."""
        N = measurement_noise(self.dimension, translation_precision, rotation_precision, len(self.pairs))
        k = np.arange(self.dof)
        w = 1.0 / np.sqrt(N[:, k, k])  # N^-1/2: det(I + N^-1 P) = det(I + N^-1/2 P N^-1/2), symmetric
        M = np.eye(self.dof)[None] + w[:, :, None] * self.covariance * w[:, None, :]
        return 0.5 * np.linalg.slogdet(M)[1]


def _pose_pair_ids(prob, pairs, who):
    """Name pairs -> (C, 2) pose ids; a landmark's name is refused."""
    ids = pair_ids(prob, pairs, who)
    for c, pair in enumerate(pairs):
        for k in range(2):
            if ids[c, k] >= prob.Np:
                raise ValueError(f"{who}: {pair[k]} is a landmark: a relative pose joins two poses")
    return ids


def _device_has_relative(lib_path) -> bool:
    return all(hasattr(load_library(lib_path), sym) for sym in RELATIVE)


def predicted_relative_poses(data, results, pairs, range_weights=None, loop_closure_weights=None, rel_tol: float = 1e-10,
                             max_iters: int = 4000, block_width: int = MAX_BLOCK_WIDTH, engine: str = "auto",
                             lib_path: Optional[str] = None, solver_settings: Optional[dict] = None):
    """The relative pose T_a^-1 T_b the estimate ``results`` predicts for every pair of pose names in ``pairs``, e.g.
    ``[("A10", "B7")]``, and its covariance G H^-1 G' under ``range_weights`` / ``loop_closure_weights`` (normally those of
    the robust result that gave ``results``): dp columns per pair, ``block_width`` consecutive columns per block of the
    marginals' PCG.  ``engine``: "device", "python" (dense H, Cholesky), or "auto": the device where the library has the call
    (the CPU twin has not).  Returns ``(PredictedRelativePoses, info)``; ``info``: ``residuals`` (C x dp,
    |G'e_q - H x|_2), ``iterations``, ``asymmetry`` (max |P - P'| of the covariances as computed), ``pcg_iters``,
    ``batches``, ``setup_ms``, ``solve_ms``, ``engine``.  A column that does not converge raises RuntimeError."""
    if engine not in ("auto", "device", "python"):
        raise ValueError("engine must be 'auto', 'device' or 'python'")
    check_block_solve(block_width, rel_tol, max_iters)
    prob, point = _problem_and_point(data, results, range_weights, loop_closure_weights)
    pairs = [tuple(p) for p in pairs]
    if not pairs:
        raise ValueError("predicted_relative_poses: no pairs")
    ids = _pose_pair_ids(prob, pairs, "predicted_relative_poses")
    d, dp = unknown_sizes(prob)
    if engine == "auto":
        engine = "device" if _device_has_relative(lib_path) else "python"
    if engine == "python":
        import scipy.linalg as sla

        G, rot, trans = relative_jacobians(prob, point, ids)
        H = dense_information(prob, point)
        try:
            X = sla.cho_solve(sla.cho_factor(H, lower=True), G)
        except (np.linalg.LinAlgError, ValueError):
            raise _singular("predicted_relative_poses", len(pairs) * dp, len(pairs) * dp, "columns", max_iters) from None
        cov = np.stack([G[:, c * dp:(c + 1) * dp].T @ X[:, c * dp:(c + 1) * dp] for c in range(len(pairs))])
        res = np.linalg.norm(G - H @ X, axis=0).reshape(len(pairs), dp)
        info = {"pcg_iters": 0, "batches": 0, "setup_ms": 0.0, "solve_ms": 0.0, "iterations": np.zeros((len(pairs), dp), dtype=np.int64)}
    else:
        with RelativeHandle(prob, lib_path, solver_settings) as h:
            out = h.relative_covariances(point, ids, rel_tol, max_iters, int(block_width))
        failed = int(np.count_nonzero(~out["converged"]))
        if failed:
            raise _singular("predicted_relative_poses", failed, len(pairs) * dp, "columns", max_iters)
        rot, trans, cov, res, rec = out["rotations"], out["translations"], out["covariances"], out["residuals"], out["info"]
        info = {"pcg_iters": int(rec["pcg_iters"]), "batches": int(rec["batches"]), "setup_ms": float(rec["setup_ms"]),
                "solve_ms": float(rec["solve_ms"]), "iterations": out["iterations"]}
    covT = np.swapaxes(cov, 1, 2)
    info.update({"residuals": res, "asymmetry": float(np.max(np.abs(cov - covT))), "engine": engine})
    return PredictedRelativePoses(pairs, rot, trans, 0.5 * (cov + covT)), info


__all__ = ["predicted_relative_poses", "PredictedRelativePoses", "RelativeHandle", "relative_jacobians", "pair_jacobian",
           "measurement_noise", "so3_log", "wrap_angle", "RELATIVE_SYMBOLS"]

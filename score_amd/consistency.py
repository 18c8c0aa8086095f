"""Consistency of an estimate with its covariance: the normalised estimation error squared (NEES).

``marginal_covariances`` / ``marginal_covariances_batch`` state a covariance in the refinement's own unknowns -- (theta, x, y)
per 2-D pose, (omega, v) of the retraction R Exp(omega), t + v per 3-D pose, the coordinates of a landmark.  ``nees`` states the
error of an estimate against the truth in those same unknowns and returns e' Sigma^-1 e per variable: for a consistent
estimator with Gaussian noise it is chi-squared with as many degrees of freedom as the variable has unknowns, so over many
worlds its mean is that number.  Pure NumPy: no device, no library.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np


def rotation_error(R_est: np.ndarray, R_true: np.ndarray) -> np.ndarray:
    """The rotation vector omega with R_est Exp(omega) = R_true, |omega| <= pi (exactly zero where the two are equal)."""
    R_est, R_true = np.asarray(R_est, dtype=np.float64), np.asarray(R_true, dtype=np.float64)
    # sin(angle) * axis: the antisymmetric part of M = R_est' R_true, written row by row so that equal inputs cancel exactly
    vec = -0.5 * np.cross(R_est, R_true, axis=1).sum(axis=0)
    s, c = float(np.linalg.norm(vec)), 0.5 * (float(np.sum(R_est * R_true)) - 1.0)
    angle = float(np.arctan2(s, c))
    if s > 1e-6:
        return vec * (angle / s)
    if c > 0.0:  # angle -> 0: angle / sin(angle) = 1 + angle^2 / 6 + ...
        return vec * (1.0 + angle * angle / 6.0)
    # angle -> pi: M + M' = 2 cos I + 2 (1 - cos) a a'; the axis from the largest diagonal entry, its sign from vec
    M = R_est.T @ R_true
    B = 0.5 * (M + M.T) - c * np.eye(3)
    k = int(np.argmax(np.diag(B)))
    axis = B[:, k] / np.sqrt(B[k, k] * (1.0 - c))
    if float(axis @ vec) < 0.0:
        axis = -axis
    return axis * angle


def so3_log(M: np.ndarray) -> np.ndarray:
    """The rotation vector omega with Exp(omega) = M (3 x 3, a rotation), |omega| <= pi."""
    return rotation_error(np.eye(3), M)


def pose_error(T_true: np.ndarray, T_est: np.ndarray) -> np.ndarray:
    """The error of a pose estimate in the unknowns its covariance is stated in (homogeneous 3 x 3 or 4 x 4 matrices):
    2-D (wrap(theta_true - theta_est), t_true - t_est); 3-D (omega, v) with R_est Exp(omega) = R_true, v = t_true - t_est."""
    T_true, T_est = np.asarray(T_true, dtype=np.float64), np.asarray(T_est, dtype=np.float64)
    d = T_true.shape[0] - 1
    if T_true.shape != (d + 1, d + 1) or T_est.shape != T_true.shape or d not in (2, 3):
        raise ValueError("pose_error: homogeneous 3 x 3 or 4 x 4 matrices expected")
    v = T_true[:d, d] - T_est[:d, d]
    if d == 2:
        dth = np.arctan2(T_true[1, 0], T_true[0, 0]) - np.arctan2(T_est[1, 0], T_est[0, 0])
        return np.concatenate([[np.arctan2(np.sin(dth), np.cos(dth))], v])
    return np.concatenate([rotation_error(T_est[:3, :3], T_true[:3, :3]), v])


def nees(truth, estimate, cov: Dict[str, np.ndarray], order: Optional[Sequence[str]] = None) -> Dict[str, Tuple[float, int]]:
    """``name -> (e' Sigma^-1 e, degrees of freedom)`` for the variables of ``order`` (None: every variable of ``cov``).
    ``truth`` and ``estimate`` are SolverResults of the same graph; ``cov`` maps names to the k x k blocks
    ``marginal_covariances`` returns."""
    out = {}
    for nm in (list(cov) if order is None else [str(v) for v in order]):
        if nm not in cov:
            raise ValueError(f"nees: no covariance for {nm}")
        S = np.asarray(cov[nm], dtype=np.float64)
        if nm in estimate.poses:
            e = pose_error(truth.poses[nm], estimate.poses[nm])
        elif nm in estimate.landmarks:
            e = np.asarray(truth.landmarks[nm], dtype=np.float64) - np.asarray(estimate.landmarks[nm], dtype=np.float64)
        else:
            raise ValueError(f"nees: unknown variable {nm}")
        if S.shape != (e.size, e.size):
            raise ValueError(f"nees: the covariance of {nm} is {S.shape[0]} x {S.shape[1]}, its error has {e.size} entries")
        out[nm] = (float(e @ np.linalg.solve(S, e)), int(e.size))
    return out


__all__ = ["nees", "pose_error", "rotation_error", "so3_log"]

"""Marginal covariances of a refined estimate (include/score_marginals.h).

At the maximum-likelihood estimate the Gauss-Newton matrix H = J'J of the cost ``refine_estimate`` minimises is the
information matrix in the refinement's own unknowns -- (theta, x, y) per 2-D pose, (omega, v) of the retraction
R Exp(omega), t + v per 3-D pose, the coordinates of a landmark; the first pose of the first chain is fixed -- and the
covariance of a set S of variables is the S x S part of H^-1.  ``marginal_covariances`` solves H X = E_S on the device
(``score_refine_marginals``: blocks of up to 16 unit columns advance in lock-step through a chain-preconditioned PCG,
one pass over H per iteration for the whole block) and returns one k x k block per variable.
``engine="python"`` is the dense inverse of J'J from the host Jacobian: for small graphs and the tests.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import MARGINALS, ScoreMarginalsInfo, bind, ptr, steps_and_converged
from .refine import RefineHandle, _point_arrays, _problem_and_point, unknown_sizes
from .solver import _i32p

# the symbols include/score_marginals.h declares
MARGINALS_SYMBOLS = list(MARGINALS)
MAX_BLOCK_WIDTH = 16


def _bind(lib: C.CDLL) -> C.CDLL:
    return bind(lib, MARGINALS)


def check_block_solve(block_width, rel_tol, max_iters, first_sample=None, n_samples=0):
    """The arguments of a block solve whose width is 1..16; ``first_sample``: of one that draws, ``n_samples`` draws at most."""
    if int(block_width) != block_width or not 1 <= int(block_width) <= MAX_BLOCK_WIDTH:
        raise ValueError(f"block_width must be an integer in 1..{MAX_BLOCK_WIDTH}")
    if first_sample is not None and (int(first_sample) != first_sample or first_sample < 0 or first_sample + n_samples > 2 ** 32):
        raise ValueError("first_sample .. first_sample + n_samples must lie in 0 .. 2^32")
    if not rel_tol > 0 or max_iters < 1:
        raise ValueError("rel_tol must be positive and max_iters at least 1")


def _select(prob, variables):
    """Names -> (names, variable ids, first column and size of each, all columns)."""
    poses, lms = list(prob.a["pose_names"]), list(prob.a["landmark_names"])
    if variables is None:
        last = np.cumsum(np.asarray(prob.a["chain_len"], dtype=np.int64)) - 1
        variables = lms + [poses[i] for i in last if i > 0]  # (a first chain of one pose has only the fixed pose)
    variables = [str(v) for v in variables]
    if not variables:
        raise ValueError("marginal_covariances: no variables")
    pose_id = {nm: i for i, nm in enumerate(poses)}
    lm_id = {nm: i for i, nm in enumerate(lms)}
    d, dp = unknown_sizes(prob)
    ids, first, size, seen = [], [], [], set()
    for nm in variables:
        if nm in seen:
            raise ValueError(f"marginal_covariances: {nm} is listed twice")
        seen.add(nm)
        if nm in pose_id:
            p = pose_id[nm]
            if p == 0:
                raise ValueError(f"marginal_covariances: {nm} is the fixed first pose, it has no covariance")
            ids.append(p); first.append(dp * (p - 1)); size.append(dp)
        elif nm in lm_id:
            l = lm_id[nm]
            ids.append(prob.Np + l); first.append(dp * (prob.Np - 1) + d * l); size.append(d)
        else:
            raise ValueError(f"marginal_covariances: unknown variable {nm}")
    cols = np.concatenate([np.arange(f, f + s) for f, s in zip(first, size)]).astype(np.int64)
    return variables, np.asarray(ids, dtype=np.int32), size, cols


def n_columns(prob, ids) -> int:
    """The unknowns of the variables ``ids`` (poses 0..Np-1, then the landmarks): the columns a call solves for them."""
    d, dp = unknown_sizes(prob)
    return int(np.where(np.asarray(ids) < prob.Np, dp, d).sum())


def dense_information(prob, point) -> np.ndarray:
    """J'J at the point as a dense matrix (small graphs, tests)."""
    _, J = prob.residuals(point, jac=True)
    return np.asarray((J.T @ J).todense(), dtype=np.float64)


def _python_columns(prob, point, cols):
    H = dense_information(prob, point)
    try:
        Sigma = np.linalg.inv(H)
    except np.linalg.LinAlgError as e:
        raise RuntimeError(f"marginal_covariances: J'J is singular ({e}): a variable is not determined by the measurements")
    X = Sigma[:, cols]
    res = np.linalg.norm(np.eye(prob.n)[:, cols] - H @ X, axis=0)
    return X[cols, :], res


class MarginalsHandle(RefineHandle):
    """A refinement handle (``score_refine_create``) kept for several ``score_refine_marginals`` calls on one graph: the
    pattern, the chain tables and the block's buffers are set up once."""

    headers = RefineHandle.headers + (MARGINALS,)

    def columns(self, point, ids, rel_tol=1e-10, max_iters=4000, block_width=MAX_BLOCK_WIDTH):
        """``score_refine_marginals`` as it is: returns (return code, C x C matrix whose column c is x_c on the selected
        rows -- not symmetrised --, residuals, steps per column, converged mask, the call's info record)."""
        prob = self.prob
        poses, lms = _point_arrays(prob, point)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        ncol = n_columns(prob, ids)
        joint = np.zeros((ncol, ncol))
        res = np.zeros(ncol)
        its = np.zeros(ncol, dtype=np.int32)
        info = ScoreMarginalsInfo()
        rc = self.lib.score_refine_marginals(self.h, ptr(poses), ptr(lms), ptr(ids, _i32p), len(ids), float(rel_tol), int(max_iters),
                                             int(block_width), ptr(joint), ptr(res), ptr(its, _i32p), C.byref(info))
        if rc < 0:
            raise RuntimeError(f"score_refine_marginals failed: {self.lib.score_last_error().decode()}")
        steps, converged = steps_and_converged(its)
        return rc, joint, res, steps, converged, info.as_dict()


def device_columns(prob, point, ids, rel_tol=1e-10, max_iters=4000, block_width=MAX_BLOCK_WIDTH, lib_path=None,
                   solver_settings=None):
    """One ``MarginalsHandle.columns`` call on a handle of its own."""
    with MarginalsHandle(prob, lib_path, solver_settings) as h:
        return h.columns(point, ids, rel_tol, max_iters, block_width)


def marginal_covariances(data, results, variables=None, joint: bool = False, range_weights=None, loop_closure_weights=None,
                         rel_tol: float = 1e-10, max_iters: int = 4000, block_width: int = MAX_BLOCK_WIDTH,
                         engine: str = "device", lib_path: Optional[str] = None, solver_settings: Optional[dict] = None):
    """Covariances of ``variables`` (pose or landmark names; None: every landmark and the last pose of every chain) at the
    estimate ``results`` -- normally what ``refine_estimate`` returned, with the same ``range_weights`` /
    ``loop_closure_weights``.  Returns ``(dict name -> k x k ndarray, info)``: k = 3 (theta, x, y) or 6 (omega, v) for a
    pose, 2 or 3 for a landmark; every block symmetrised as (A + A')/2.  ``info``: ``order`` (the names), ``residuals``
    (|e_c - H x_c|_2 per column), ``iterations``, ``asymmetry`` (max |A - A'| of the matrix as computed), ``pcg_iters``,
    ``batches``, ``setup_ms``, ``solve_ms`` and, with ``joint=True``, ``joint`` (the symmetrised matrix of all selected
    variables, in ``order``) and ``joint_raw`` (column c as computed).
    ``block_width``: 1..16 columns advance together; 0 solves one column at a time with the single-right-hand-side PCG.
    A column that does not converge raises RuntimeError naming its variable: usually one the measurements do not determine."""
    if engine not in ("device", "python"):
        raise ValueError("engine must be 'device' or 'python'")
    if int(block_width) != block_width or not 0 <= int(block_width) <= MAX_BLOCK_WIDTH:
        raise ValueError(f"block_width must be an integer in 0..{MAX_BLOCK_WIDTH}")
    if not rel_tol > 0 or max_iters < 1:
        raise ValueError("rel_tol must be positive and max_iters at least 1")
    prob, point = _problem_and_point(data, results, range_weights, loop_closure_weights)
    names, ids, size, cols = _select(prob, variables)
    if engine == "python":
        A, res = _python_columns(prob, point, cols)
        steps = np.zeros(len(cols), dtype=np.int64)
        converged = np.isfinite(res)
        rec = {"pcg_iters": 0, "batches": 0, "setup_ms": 0.0, "solve_ms": 0.0}
    else:
        _, A, res, steps, converged, rec = device_columns(prob, point, ids, rel_tol, max_iters, int(block_width), lib_path,
                                                          solver_settings)
    return _member_result("marginal_covariances", None, names, size, A, res, steps, converged, rec, engine, joint, max_iters)


def _member_result(who, where, names, size, A, res, steps, converged, rec, engine, joint, max_iters):
    """``(covariances, info)`` of one graph from its columns.  ``who`` and ``where`` (None: nothing) open the message about
    columns that did not converge."""
    off = np.concatenate([[0], np.cumsum(size)])
    if not np.all(converged):
        bad = [nm for k, nm in enumerate(names) if not np.all(converged[off[k]:off[k + 1]])]
        at = f"{who}: {where}: " if where else f"{who}: "
        raise RuntimeError(f"{at}the columns of {', '.join(bad)} did not converge in {max_iters} iterations "
                           "(a variable the measurements do not determine?)")
    S = 0.5 * (A + A.T)
    out = {nm: S[off[k]:off[k + 1], off[k]:off[k + 1]].copy() for k, nm in enumerate(names)}
    info = {"order": names, "residuals": res, "iterations": steps, "asymmetry": float(np.max(np.abs(A - A.T))),
            "pcg_iters": int(rec["pcg_iters"]), "batches": int(rec["batches"]), "setup_ms": float(rec["setup_ms"]),
            "solve_ms": float(rec["solve_ms"]), "engine": engine}
    if joint:
        info["joint"] = S
        info["joint_raw"] = A
    return out, info


__all__ = ["marginal_covariances", "MarginalsHandle", "device_columns", "dense_information", "MARGINALS_SYMBOLS", "MAX_BLOCK_WIDTH"]

"""Greedy selection of candidate loop closures by joint information gain at a refined estimate
(include/score_select_poses.h): the block form of ``select_ranges``.

``predicted_relative_poses(...).information_gain(...)`` says what ONE hypothetical relative pose would be worth.  Loop closures
are the measurements that cost the most to obtain -- a place-recognition match to verify, a rendezvous to plan -- and the most
redundant candidates: ten matches between two passes through one corridor are nearly one measurement, so a ranking by the
single gain picks redundant sets.  For the Gaussian posterior at the estimate, the set S of relative poses with translation
precisions kappa_c and rotation precisions tau_c gains

    gain(S) = 1/2 [logdet(H + sum_{c in S} G_c' N_c^-1 G_c) - logdet H] = 1/2 logdet A_SS,
    A = I + D (P + P')/2 D,   P = G H^-1 G' (N x N, N = C dp columns r = c dp + q),   D = diag(sqrt w),

with N_c = diag(I / (2 tau_c), I / kappa_c) of ``relative.measurement_noise``, i.e. w_r = 2 tau_c for the rotation coordinates
and kappa_c for the translation coordinates.  The gain is monotone and submodular, so the greedy rule is within 1 - 1/e of the
best set of its size.  A candidate is a block of dp = 3 or 6 columns: the rule is a block-pivoted Cholesky factorisation of A
whose pivot is the dp x dp Schur block B_c = I + D_c Sigma_{c|S} D_c, scored by 1/2 logdet B_c
(csrc/score_select_poses_rule.hpp states it in full).

``select_loop_closures`` runs it on the device (``score_refine_select_relative_poses``): the columns of
``predicted_relative_poses``, one small kernel per solved block for the cross terms, one launch for the factorisation.
``engine="python"`` is the dense H and ``block_greedy_reference``, the NumPy restatement of the rule: small graphs, the tests.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import SELECT_POSES, ScoreSelectPosesInfo, bind, ptr, steps_and_converged
from .leverage import _check_block
from .marginals import MAX_BLOCK_WIDTH, _problem_and_point, dense_information
from .refine import _point_arrays, unknown_sizes
from .relative import _pose_pair_ids, relative_jacobians
from .selection import MAX_CANDIDATES, MAX_PICKS, SelectionHandle, selection_matrix
from .solver import _i32p, load_library

# the symbols include/score_select_poses.h declares
SELECT_POSES_SYMBOLS = list(SELECT_POSES)


def _bind(lib: C.CDLL) -> C.CDLL:
    return bind(lib, SELECT_POSES)


def column_precisions(d, translation_precisions, rotation_precisions, count):
    """w (count dp): the precisions of the columns r = c dp + q -- 2 tau_c for the rotation coordinates (q < dp - d), kappa_c
    for the translation coordinates: the inverse diagonal of ``relative.measurement_noise``."""
    dp = 3 if d == 2 else 6
    kappa = np.broadcast_to(np.asarray(translation_precisions), (count,))
    tau = np.broadcast_to(np.asarray(rotation_precisions), (count,))
    rot = (np.arange(dp) < dp - d)[None, :]
    return np.where(rot, 2 * tau[:, None], kappa[:, None]).reshape(count * dp)


def _block_gains(B):
    """selp_gain of every block of B (C x dp x dp) in B's dtype: the unpivoted Cholesky factorisation with q ascending, every
    sum subtracted term by term with m ascending; 0 where a pivot is not > 0, else 1/2 of the logs added with q ascending."""
    n, dp = B.shape[0], B.shape[1]
    c = np.zeros_like(B)
    s = np.zeros(n, dtype=B.dtype)
    ok = np.ones(n, dtype=bool)
    one = B.dtype.type(1)
    for q in range(dp):
        pi = B[:, q, q].copy()
        for m in range(q):
            pi = pi - c[:, q, m] * c[:, q, m]
        ok &= pi > 0
        safe = np.where(ok, pi, one)
        lg = np.log(safe)
        s = lg if q == 0 else s + lg
        root = np.sqrt(safe)
        for i in range(q + 1, dp):
            acc = B[:, i, q].copy()
            for m in range(q):
                acc = acc - c[:, i, m] * c[:, q, m]
            c[:, i, q] = acc / root
    return np.where(ok, s / 2, 0 * s)


def _scaled(B, w):
    """selp_scaled of the blocks B (.. x dp x dp) with the columns' precisions w (.. x dp): (B - I) / (sqrt w sqrt w')."""
    sw = np.sqrt(w)
    return (B - np.eye(B.shape[-1], dtype=B.dtype)) / (sw[..., :, None] * sw[..., None, :])


def block_greedy_reference(P, w, dp, k, min_gain=0.0, excluded=None, dtype=np.float64) -> dict:
    """The rule of csrc/score_select_poses_rule.hpp in NumPy, in ``dtype``, on P (N x N, N = C dp) with the columns'
    precisions ``w`` (N): ``order`` (k, padded with -1), ``gains`` (k, padded with 0), ``pick_covariances`` (k x dp x dp,
    padded with 0), ``remaining`` (C x dp x dp; a picked candidate: the value at its pick), ``picked``, ``asymmetry``
    (max |P_rs - P_sr|) and ``min_gap``: the smallest relative gap (gain_p - gain_next) / gain_p between the two best eligible
    candidates over the steps taken (inf where a step had one eligible candidate)."""
    P = np.asarray(P, dtype=dtype)
    w = np.asarray(w, dtype=dtype)
    N = len(w)
    n = N // dp
    assert n * dp == N and P.shape == (N, N)
    A = selection_matrix(P, w)
    wb = w.reshape(n, dp)
    state = np.ones(n, dtype=np.int64)  # 0 excluded, 1 eligible, 2 picked
    if excluded is not None:
        state[np.asarray(excluded) != 0] = 0
    idx = np.arange(n)
    B = np.stack([A[c * dp:(c + 1) * dp, c * dp:(c + 1) * dp] for c in range(n)]).copy()
    L = np.zeros((N, k * dp), dtype=dtype)
    order = np.full(k, -1, dtype=np.int32)
    gains = np.zeros(k, dtype=dtype)
    pick = np.zeros((k, dp, dp), dtype=dtype)
    remaining = np.zeros((n, dp, dp), dtype=dtype)
    min_gap, j = np.inf, 0
    while j < k:
        eligible = idx[state == 1]
        if eligible.size == 0:
            break
        g = _block_gains(B[eligible])
        at = int(np.argmax(g))  # (the first of equal maxima: the lowest index)
        p, gp = int(eligible[at]), g[at]
        if not gp > 0 or gp < min_gain:
            break
        if eligible.size > 1:
            min_gap = min(min_gap, float((gp - np.max(np.delete(g, at))) / gp))
        order[j], gains[j] = p, gp
        pick[j] = remaining[p] = _scaled(B[p], wb[p])
        state[p] = 2
        for q in range(dp):
            J, r = j * dp + q, p * dp + q
            acc = A[r, :].copy()
            for m in range(J):
                acc -= L[:, m] * L[r, m]
            l = acc / np.sqrt(B[p, q, q])
            L[:, J] = l
            lb = l.reshape(n, dp)
            B -= lb[:, :, None] * lb[:, None, :]
        j += 1
    left = state != 2
    remaining[left] = _scaled(B[left], wb[left])
    return {"order": order, "gains": gains, "pick_covariances": pick, "remaining": remaining, "picked": int(j),
            "asymmetry": float(np.max(np.abs(P - P.T))), "min_gap": min_gap}


def _check_pose_selection(n, dp, k, min_gain, kappa, tau, who):
    if n < 1 or n > MAX_CANDIDATES // dp:
        raise ValueError(f"{who}: the number of candidates must be 1..{MAX_CANDIDATES // dp}")
    if int(k) != k or k < 1 or k > min(n, MAX_PICKS // dp):
        raise ValueError(f"{who}: k must be 1..min(candidates, {MAX_PICKS // dp})")
    if not min_gain >= 0:
        raise ValueError(f"{who}: min_gain must be >= 0")
    for w in (kappa, tau):
        if w.shape != (n,) or not np.all(np.isfinite(w)) or not np.all(w > 0):
            raise ValueError(f"{who}: one finite, positive precision per candidate (or one for all)")


def block_greedy_from_matrix(P, translation_precisions, rotation_precisions, dim, k, min_gain=0.0, excluded=None,
                             lib_path: Optional[str] = None) -> dict:
    """``score_select_block_greedy`` as it is: the selection alone on the matrix ``P`` (N x N, N = C dp; (P + P')/2 is used)
    on the device, ``dim`` = 2 or 3.  Returns what ``block_greedy_reference`` returns, without ``min_gap``, and ``rc``."""
    lib = _bind(load_library(lib_path))
    dp = 3 if dim == 2 else 6
    P = np.ascontiguousarray(P, dtype=np.float64)
    kappa = np.ascontiguousarray(translation_precisions, dtype=np.float64)
    tau = np.ascontiguousarray(rotation_precisions, dtype=np.float64)
    n = len(kappa)
    ex = None if excluded is None else np.ascontiguousarray(excluded, dtype=np.int32)
    kk = max(int(k), 0)
    order = np.full(kk, -7, dtype=np.int32)
    gains, pick, remaining = np.zeros(kk), np.zeros((kk, dp, dp)), np.zeros((n, dp, dp))
    picked, asym = C.c_int32(-1), C.c_double(-1.0)
    rc = lib.score_select_block_greedy(ptr(P), ptr(kappa), ptr(tau), ptr(ex, _i32p), n, int(dim), int(k), float(min_gain),
                                       ptr(order, _i32p), ptr(gains), ptr(pick), ptr(remaining), C.byref(picked), C.byref(asym))
    if rc < 0:
        raise RuntimeError(f"score_select_block_greedy failed: {lib.score_last_error().decode()}")
    return {"rc": rc, "order": order, "gains": gains, "pick_covariances": pick, "remaining": remaining, "picked": int(picked.value),
            "asymmetry": float(asym.value)}


class PoseSelectionHandle(SelectionHandle):
    """A refinement handle kept for ``score_refine_select_relative_poses`` calls on one graph (and, being a
    ``SelectionHandle``, for every analysis before it)."""

    headers = SelectionHandle.headers + (SELECT_POSES,)

    def select_relative_poses(self, point, pair_ids, translation_precisions, rotation_precisions, k, min_gain=0.0, rel_tol=1e-10,
                              max_iters=4000, block_width=MAX_BLOCK_WIDTH, with_matrix=False) -> dict:
        """``score_refine_select_relative_poses`` as it is.  ``pair_ids``: (C, 2) pose ids; the precisions: C each.  Returns a
        dict: ``rc``, ``order``, ``gains`` (k each), ``pick_covariances`` (k x dp x dp), ``rotations``, ``translations``,
        ``covariances``, ``residuals``, ``iterations``, ``converged`` (as ``relative_covariances``), ``remaining``
        (C x dp x dp), ``matrix`` (asked for: C dp x C dp, P as computed; else None) and ``info``."""
        d, dp = unknown_sizes(self.prob)
        poses, lms = _point_arrays(self.prob, point)
        pairs = np.asarray(pair_ids, dtype=np.int32).reshape(-1, 2)
        pa, pb = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        kappa = np.ascontiguousarray(translation_precisions, dtype=np.float64)
        tau = np.ascontiguousarray(rotation_precisions, dtype=np.float64)
        n, kk = len(pa), max(int(k), 0)
        order = np.full(kk, -7, dtype=np.int32)
        gains, pick = np.zeros(kk), np.zeros((kk, dp, dp))
        rot, trans, cov, rem = np.zeros((n, d, d)), np.zeros((n, d)), np.zeros((n, dp, dp)), np.zeros((n, dp, dp))
        res, its = np.zeros((n, dp)), np.zeros((n, dp), dtype=np.int32)
        mat = np.zeros((n * dp, n * dp)) if with_matrix else None
        info = ScoreSelectPosesInfo()
        rc = self.lib.score_refine_select_relative_poses(self.h, ptr(poses), ptr(lms), ptr(pa, _i32p), ptr(pb, _i32p), ptr(kappa),
                                                         ptr(tau), n, int(k), float(min_gain), float(rel_tol), int(max_iters),
                                                         int(block_width), ptr(order, _i32p), ptr(gains), ptr(pick), ptr(rot),
                                                         ptr(trans), ptr(cov), ptr(rem), ptr(res), ptr(its, _i32p), ptr(mat),
                                                         C.byref(info))
        if rc < 0:
            raise RuntimeError(f"score_refine_select_relative_poses failed: {self.lib.score_last_error().decode()}")
        iterations, converged = steps_and_converged(its)
        return {"rc": rc, "order": order, "gains": gains, "pick_covariances": pick, "rotations": rot, "translations": trans,
                "covariances": cov, "remaining": rem, "residuals": res, "iterations": iterations, "converged": converged,
                "matrix": mat, "info": info.as_dict()}


class PoseSelection:
    """The greedy selection among ``candidates`` (pairs of pose names): ``order`` (indices into the candidates, in the order of
    the picks), ``pairs`` (the picked pairs in that order), ``gains`` (nats per pick: non-increasing), ``total_gain`` (the gain
    of the picked set), ``pick_covariance`` (picks x dp x dp: the covariance of each pick's error coordinates given the picks
    before it), ``rotation``, ``translation`` and ``covariance`` (per candidate, as ``PredictedRelativePoses``),
    ``remaining_covariance`` (per candidate: its covariance once the picks are measured; NaN at the picked ones),
    ``remaining_gain`` (per candidate: what it would still add, 1/2 logdet(I + N^-1 remaining_covariance); NaN at the picked
    ones) and ``excluded`` (indices of candidates with a column that did not converge: never picked)."""

    def __init__(self, candidates, order, gains, pick_covariance, rotation, translation, covariance, remaining, column_w, excluded):
        self.candidates = list(candidates)
        self.order = np.asarray(order, dtype=np.int64)
        self.pairs = [self.candidates[c] for c in self.order]
        self.gains = np.asarray(gains, dtype=np.float64)
        self.total_gain = float(np.sum(self.gains))
        self.pick_covariance = np.asarray(pick_covariance, dtype=np.float64)
        self.rotation = np.asarray(rotation, dtype=np.float64)
        self.translation = np.asarray(translation, dtype=np.float64)
        cov = np.asarray(covariance, dtype=np.float64)
        self.covariance = 0.5 * (cov + np.swapaxes(cov, 1, 2))
        self.dimension = self.translation.shape[1]
        self.dof = 3 if self.dimension == 2 else 6
        self.remaining_covariance = np.array(remaining, dtype=np.float64)
        sw = np.sqrt(np.asarray(column_w, dtype=np.float64).reshape(len(self.candidates), self.dof))
        M = np.eye(self.dof)[None] + sw[:, :, None] * self.remaining_covariance * sw[:, None, :]
        self.remaining_gain = 0.5 * np.linalg.slogdet(M)[1]
        self.remaining_covariance[self.order] = np.nan
        self.remaining_gain[self.order] = np.nan
        self.excluded = np.asarray(excluded, dtype=np.int64)


def select_loop_closures(data, results, pairs, k: int, translation_precision=1.0, rotation_precision=1.0, min_gain: float = 0.0,
                         range_weights=None, loop_closure_weights=None, rel_tol: float = 1e-10, max_iters: int = 4000,
                         block_width: int = MAX_BLOCK_WIDTH, engine: str = "device", lib_path: Optional[str] = None,
                         solver_settings: Optional[dict] = None):
    """The ``k`` of the candidate loop closures ``pairs`` (pairs of pose names, e.g. ``[("A10", "B7")]``) that the greedy rule
    picks at the estimate ``results``, each a relative pose of ``translation_precision`` (kappa) and ``rotation_precision``
    (tau) -- the loop closures' attributes; one number, or one per candidate; the rule stops early where the next pick would
    add less than ``min_gain`` nats.  Returns ``(PoseSelection, info)``; ``info``: ``residuals`` (C x dp, |G'e_q - H x|_2),
    ``iterations``, ``pcg_iters``, ``batches``, ``setup_ms``, ``solve_ms``, ``cross_ms``, ``greedy_ms``, ``asymmetry``
    (max |P_rs - P_sr| as computed), ``engine``.  A candidate with a column that does not converge is excluded."""
    _check_block(block_width, rel_tol, max_iters, engine)
    prob, point = _problem_and_point(data, results, range_weights, loop_closure_weights)
    pairs = [tuple(p) for p in pairs]
    if not pairs:
        raise ValueError("select_loop_closures: no pairs")
    ids = _pose_pair_ids(prob, pairs, "select_loop_closures")
    d, dp = unknown_sizes(prob)
    n = len(pairs)
    kappa, tau = (np.asarray(v, dtype=np.float64) for v in (translation_precision, rotation_precision))
    kappa = np.full(n, float(kappa)) if kappa.ndim == 0 else kappa.copy()
    tau = np.full(n, float(tau)) if tau.ndim == 0 else tau.copy()
    _check_pose_selection(n, dp, k, min_gain, kappa, tau, "select_loop_closures")
    w = column_precisions(d, kappa, tau, n)
    if engine == "python":
        import scipy.linalg as sla

        G, rot, trans = relative_jacobians(prob, point, ids)
        H = dense_information(prob, point)
        try:
            X = sla.cho_solve(sla.cho_factor(H, lower=True), G)
        except (np.linalg.LinAlgError, ValueError):
            raise RuntimeError("select_loop_closures: J'J is singular -- information_spectrum(...).undetermined() names the "
                               "variables the measurements do not determine") from None
        P = G.T @ X
        out = block_greedy_reference(P, w, dp, int(k), float(min_gain))
        cov = np.stack([P[c * dp:(c + 1) * dp, c * dp:(c + 1) * dp] for c in range(n)])
        excluded = np.zeros(0, dtype=np.int64)
        info = {"pcg_iters": 0, "batches": 0, "setup_ms": 0.0, "solve_ms": 0.0, "cross_ms": 0.0, "greedy_ms": 0.0,
                "iterations": np.zeros((n, dp), dtype=np.int64), "residuals": np.linalg.norm(G - H @ X, axis=0).reshape(n, dp),
                "asymmetry": out["asymmetry"]}
    else:
        with PoseSelectionHandle(prob, lib_path, solver_settings) as h:
            out = h.select_relative_poses(point, ids, kappa, tau, int(k), float(min_gain), rel_tol, max_iters, int(block_width))
        rot, trans, cov, rec = out["rotations"], out["translations"], out["covariances"], out["info"]
        excluded = np.flatnonzero(~np.all(out["converged"], axis=1))
        info = {"pcg_iters": int(rec["solve"]["pcg_iters"]), "batches": int(rec["solve"]["batches"]),
                "setup_ms": float(rec["solve"]["setup_ms"]), "solve_ms": float(rec["solve"]["solve_ms"]),
                "cross_ms": float(rec["cross_ms"]), "greedy_ms": float(rec["greedy_ms"]), "iterations": out["iterations"],
                "residuals": out["residuals"], "asymmetry": float(rec["asymmetry"])}
        out["picked"] = int(rec["picked"])
    info["engine"] = engine
    m = out["picked"]
    sel = PoseSelection(pairs, out["order"][:m], out["gains"][:m], out["pick_covariances"][:m], rot, trans, cov, out["remaining"], w,
                        excluded)
    return sel, info


__all__ = ["select_loop_closures", "PoseSelection", "PoseSelectionHandle", "block_greedy_from_matrix", "block_greedy_reference",
           "column_precisions", "SELECT_POSES_SYMBOLS"]

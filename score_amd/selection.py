"""Greedy selection of candidate ranges by joint information gain at a refined estimate (include/score_select.h).

``predicted_range_variances`` says what ONE hypothetical range would be worth, ``PredictedRanges.information_gain`` =
1/2 log(1 + w sigma^2).  The question of active ranging is another: "k more ranges out of these C candidates -- which k?"  The
single gains do not add: two candidates at neighbouring poses are nearly the same measurement, and a ranking by the
individual gain picks redundant sets.  For the Gaussian posterior at the estimate, the set S of ranges with precisions w_c
gains

    gain(S) = 1/2 [logdet(H + sum_{c in S} w_c g_c g_c') - logdet H] = 1/2 logdet(I + D_S P_SS D_S),   P = G'H^-1 G, D = diag(sqrt w)

which is monotone and submodular, so the greedy rule is within 1 - 1/e of the best set of its size.  The rule is a diagonally
pivoted Cholesky factorisation of A = I + D (P + P')/2 D: after the picks S the Schur-complement diagonal is
d_c = 1 + w_c sigma^2_{c|S}, sigma^2_{c|S} = g_c'(H + G_S W_S G_S')^-1 g_c (Woodbury), and the next pick p adds 1/2 log d_p.

``select_ranges`` runs it on the device (``score_refine_select_ranges``): the columns of ``predicted_range_variances``, one
small kernel per solved block for the cross terms g_c'x_d, one launch for the factorisation.  ``engine="python"`` is the dense
H and ``greedy_reference``, the NumPy restatement of the rule (csrc/score_select_rule.hpp): small graphs, the tests.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import SELECT, ScoreSelectInfo, bind, ptr, steps_and_converged
from .leverage import _check_block, pair_gradients, pair_ids
from .marginals import MAX_BLOCK_WIDTH, _problem_and_point, dense_information
from .refine import _point_arrays
from .relative import RelativeHandle
from .solver import _i32p, load_library

# the symbols include/score_select.h declares
SELECT_SYMBOLS = list(SELECT)
MAX_CANDIDATES, MAX_PICKS = 4096, 256


def _bind(lib: C.CDLL) -> C.CDLL:
    return bind(lib, SELECT)


def selection_matrix(P, w):
    """A = I + D (P + P')/2 D, D = diag(sqrt w), in the dtype of P: an entry is formed once per unordered pair of indices,
    (sqrt w_lo * s) * sqrt w_hi, so A is symmetric bit for bit (the order of k_sel_sym)."""
    P = np.asarray(P)
    sw = np.sqrt(np.asarray(w, dtype=P.dtype))
    U = np.triu((sw[:, None] * (0.5 * (P + P.T))) * sw[None, :])
    A = U + np.triu(U, 1).T
    A[np.diag_indices_from(A)] = 1.0 + np.diag(U)
    return A


def greedy_reference(P, w, k, min_gain=0.0, excluded=None, dtype=np.float64) -> dict:
    """The rule of csrc/score_select_rule.hpp in NumPy, in ``dtype``: ``order`` (k, padded with -1), ``gains`` and
    ``pick_variances`` (k, padded with 0), ``remaining`` (C; a picked candidate: the value at its pick), ``picked``,
    ``asymmetry`` (max |P_cd - P_dc|) and ``min_gap``: the smallest relative gap (d_p - d_q) / d_p between the two best
    eligible pivots over the steps taken (inf where a step had one eligible candidate)."""
    P = np.asarray(P, dtype=dtype)
    w = np.asarray(w, dtype=dtype)
    n = len(w)
    A = selection_matrix(P, w)
    state = np.ones(n, dtype=np.int64)  # 0 excluded, 1 eligible, 2 picked
    if excluded is not None:
        state[np.asarray(excluded) != 0] = 0
    d = np.diag(A).copy()
    L = np.zeros((n, k), dtype=dtype)
    order = np.full(k, -1, dtype=np.int32)
    gains, pick = np.zeros(k, dtype=dtype), np.zeros(k, dtype=dtype)
    remaining = np.zeros(n, dtype=dtype)
    min_gap, j = np.inf, 0
    while j < k:
        eligible = np.flatnonzero(state == 1)
        if eligible.size == 0:
            break
        p = int(eligible[np.argmax(d[eligible])])  # (the first of equal maxima: the lowest index)
        dp = d[p]
        if not dp > 1 or 0.5 * np.log(dp) < min_gain:
            break
        others = eligible[eligible != p]
        if others.size:
            min_gap = min(min_gap, float((dp - np.max(d[others])) / dp))
        order[j], gains[j], pick[j] = p, 0.5 * np.log(dp), (dp - 1) / w[p]
        remaining[p] = pick[j]
        state[p] = 2
        acc = A[p, :].copy()
        for i in range(j):
            acc -= L[:, i] * L[p, i]
        l = acc / np.sqrt(dp)
        L[:, j] = l
        d -= l * l
        j += 1
    left = state != 2
    remaining[left] = (d[left] - 1) / w[left]
    return {"order": order, "gains": gains, "pick_variances": pick, "remaining": remaining, "picked": int(j),
            "asymmetry": float(np.max(np.abs(P - P.T))), "min_gap": min_gap}


def _check_selection(n, k, min_gain, w, who):
    if n < 1 or n > MAX_CANDIDATES:
        raise ValueError(f"{who}: the number of candidates must be 1..{MAX_CANDIDATES}")
    if int(k) != k or k < 1 or k > min(n, MAX_PICKS):
        raise ValueError(f"{who}: k must be 1..min(candidates, {MAX_PICKS})")
    if not min_gain >= 0:
        raise ValueError(f"{who}: min_gain must be >= 0")
    if w.shape != (n,) or not np.all(np.isfinite(w)) or not np.all(w > 0):
        raise ValueError(f"{who}: one finite, positive precision per candidate (or one for all)")


def greedy_from_matrix(P, precisions, k, min_gain=0.0, excluded=None, lib_path: Optional[str] = None) -> dict:
    """``score_select_greedy`` as it is: the selection alone on the matrix ``P`` (C x C, (P + P')/2 is used) on the device.
    Returns what ``greedy_reference`` returns, without ``min_gap``, and ``rc``."""
    lib = _bind(load_library(lib_path))
    P = np.ascontiguousarray(P, dtype=np.float64)
    w = np.ascontiguousarray(precisions, dtype=np.float64)
    n = len(w)
    ex = None if excluded is None else np.ascontiguousarray(excluded, dtype=np.int32)
    order = np.full(max(int(k), 0), -7, dtype=np.int32)
    gains, pick, remaining = np.zeros(len(order)), np.zeros(len(order)), np.zeros(n)
    picked, asym = C.c_int32(-1), C.c_double(-1.0)
    rc = lib.score_select_greedy(ptr(P), ptr(w), ptr(ex, _i32p), n, int(k), float(min_gain), ptr(order, _i32p), ptr(gains), ptr(pick),
                                 ptr(remaining), C.byref(picked), C.byref(asym))
    if rc < 0:
        raise RuntimeError(f"score_select_greedy failed: {lib.score_last_error().decode()}")
    return {"rc": rc, "order": order, "gains": gains, "pick_variances": pick, "remaining": remaining, "picked": int(picked.value),
            "asymmetry": float(asym.value)}


class SelectionHandle(RelativeHandle):
    """A refinement handle kept for ``score_refine_select_ranges`` calls on one graph (and, being a ``RelativeHandle``, for
    every analysis before it)."""

    headers = RelativeHandle.headers + (SELECT,)

    def select_ranges(self, point, pair_ids, precisions, k, min_gain=0.0, rel_tol=1e-10, max_iters=4000,
                      block_width=MAX_BLOCK_WIDTH, with_matrix=False) -> dict:
        """``score_refine_select_ranges`` as it is.  ``pair_ids``: (C, 2) variable ids; ``precisions``: C.  Returns a dict:
        ``rc``, ``order``, ``gains``, ``pick_variances`` (k each), ``variances``, ``distances``, ``remaining``, ``residuals``,
        ``iterations``, ``converged`` (C each), ``matrix`` (asked for: C x C, P as computed; else None) and ``info``."""
        poses, lms = _point_arrays(self.prob, point)
        pairs = np.asarray(pair_ids, dtype=np.int32).reshape(-1, 2)
        pa, pb = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        w = np.ascontiguousarray(precisions, dtype=np.float64)
        n, kk = len(pa), max(int(k), 0)
        order = np.full(kk, -7, dtype=np.int32)
        gains, pick = np.zeros(kk), np.zeros(kk)
        var, dist, rem, res = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        its = np.zeros(n, dtype=np.int32)
        mat = np.zeros((n, n)) if with_matrix else None
        info = ScoreSelectInfo()
        rc = self.lib.score_refine_select_ranges(self.h, ptr(poses), ptr(lms), ptr(pa, _i32p), ptr(pb, _i32p), ptr(w), n, int(k),
                                                 float(min_gain), float(rel_tol), int(max_iters), int(block_width),
                                                 ptr(order, _i32p), ptr(gains), ptr(pick), ptr(var), ptr(dist), ptr(rem), ptr(res),
                                                 ptr(its, _i32p), ptr(mat), C.byref(info))
        if rc < 0:
            raise RuntimeError(f"score_refine_select_ranges failed: {self.lib.score_last_error().decode()}")
        iterations, converged = steps_and_converged(its)
        return {"rc": rc, "order": order, "gains": gains, "pick_variances": pick, "variances": var, "distances": dist,
                "remaining": rem, "residuals": res, "iterations": iterations, "converged": converged, "matrix": mat,
                "info": info.as_dict()}


class Selection:
    """The greedy selection among ``candidates`` (pairs of names): ``order`` (indices into the candidates, in the order of the
    picks), ``pairs`` (the picked pairs in that order), ``gains`` (nats per pick: non-increasing), ``total_gain`` (the gain of
    the picked set), ``pick_variance`` (the variance of each pick given the picks before it), ``variance`` and ``distance``
    (per candidate: g'H^-1 g and |p_a - p_b|, as ``PredictedRanges``), ``remaining_variance`` (per candidate: its variance once
    the picks are measured; NaN at the picked ones) and ``excluded`` (indices of candidates whose column did not converge:
    never picked)."""

    def __init__(self, candidates, order, gains, pick_variance, variance, distance, remaining, excluded):
        self.candidates = list(candidates)
        self.order = np.asarray(order, dtype=np.int64)
        self.pairs = [self.candidates[c] for c in self.order]
        self.gains = np.asarray(gains, dtype=np.float64)
        self.total_gain = float(np.sum(self.gains))
        self.pick_variance = np.asarray(pick_variance, dtype=np.float64)
        self.variance, self.distance = np.asarray(variance, dtype=np.float64), np.asarray(distance, dtype=np.float64)
        self.remaining_variance = np.array(remaining, dtype=np.float64)
        self.remaining_variance[self.order] = np.nan
        self.excluded = np.asarray(excluded, dtype=np.int64)


def select_ranges(data, results, pairs, k: int, precision=1.0, min_gain: float = 0.0, range_weights=None,
                  loop_closure_weights=None, rel_tol: float = 1e-10, max_iters: int = 4000, block_width: int = MAX_BLOCK_WIDTH,
                  engine: str = "device", lib_path: Optional[str] = None, solver_settings: Optional[dict] = None):
    """The ``k`` of the candidate ranges ``pairs`` (pairs of names, e.g. ``[("A10", "L1"), ("A10", "B10")]``) that the greedy
    rule picks at the estimate ``results``, each of precision ``precision`` (one number, or one per candidate); the rule stops
    early where the next pick would add less than ``min_gain`` nats.  Returns ``(Selection, info)``; ``info``: ``residuals``
    (|g_c - H x_c|_2), ``iterations``, ``pcg_iters``, ``batches``, ``setup_ms``, ``solve_ms``, ``cross_ms``, ``greedy_ms``,
    ``asymmetry`` (max |P_cd - P_dc| as computed), ``engine``.  A column that does not converge excludes its candidate."""
    _check_block(block_width, rel_tol, max_iters, engine)
    prob, point = _problem_and_point(data, results, range_weights, loop_closure_weights)
    pairs = [tuple(p) for p in pairs]
    if not pairs:
        raise ValueError("select_ranges: no pairs")
    ids = pair_ids(prob, pairs, "select_ranges")
    w = np.asarray(precision, dtype=np.float64)
    w = np.full(len(pairs), float(w)) if w.ndim == 0 else w.copy()
    _check_selection(len(pairs), k, min_gain, w, "select_ranges")
    if engine == "python":
        G, dist = pair_gradients(prob, point, ids)
        H = dense_information(prob, point)
        try:
            X = np.linalg.solve(H, G)
        except np.linalg.LinAlgError:
            raise RuntimeError("select_ranges: J'J is singular -- information_spectrum(...).undetermined() names the variables "
                               "the measurements do not determine") from None
        P = G.T @ X
        out = greedy_reference(P, w, int(k), float(min_gain))
        var, excluded = np.diag(P).copy(), np.zeros(0, dtype=np.int64)
        info = {"pcg_iters": 0, "batches": 0, "setup_ms": 0.0, "solve_ms": 0.0, "cross_ms": 0.0, "greedy_ms": 0.0,
                "iterations": np.zeros(len(pairs), dtype=np.int64), "residuals": np.linalg.norm(G - H @ X, axis=0),
                "asymmetry": out["asymmetry"]}
    else:
        with SelectionHandle(prob, lib_path, solver_settings) as h:
            out = h.select_ranges(point, ids, w, int(k), float(min_gain), rel_tol, max_iters, int(block_width))
        var, dist, rec = out["variances"], out["distances"], out["info"]
        excluded = np.flatnonzero(~out["converged"])
        info = {"pcg_iters": int(rec["solve"]["pcg_iters"]), "batches": int(rec["solve"]["batches"]),
                "setup_ms": float(rec["solve"]["setup_ms"]), "solve_ms": float(rec["solve"]["solve_ms"]),
                "cross_ms": float(rec["cross_ms"]), "greedy_ms": float(rec["greedy_ms"]), "iterations": out["iterations"],
                "residuals": out["residuals"], "asymmetry": float(rec["asymmetry"])}
        out["picked"] = int(rec["picked"])
    info["engine"] = engine
    m = out["picked"]
    sel = Selection(pairs, out["order"][:m], out["gains"][:m], out["pick_variances"][:m], var, dist, out["remaining"], excluded)
    return sel, info


__all__ = ["select_ranges", "Selection", "SelectionHandle", "greedy_from_matrix", "greedy_reference", "selection_matrix",
           "SELECT_SYMBOLS"]

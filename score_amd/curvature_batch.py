"""The second-order check of many refined estimates at once (include/score_curvature_batch.h,
csrc/score_curvature_batch.hpp).

``hessian_spectrum`` takes one graph, builds one refinement handle and reads a 48 x 48 pencil back to the host in every
iteration.  "Did this world's refinement stop at a minimum or at a saddle?" is asked of every world of a study:
``hessian_spectrum_batch`` hands the graphs to the device as groups, by the rule of ``score_amd/groups.py``.  E_g, half the
Hessian of member g's cost, lives on the member's part of the group's union pattern, so the lock-step rounds of
``information_spectrum_batch`` carry it: the product reads E_g + sigma_g I, the device Rayleigh-Ritz step lets the lowest value
be negative, the preconditioner stays that of J'J + sigma_g I (``score_refine_batch_curvature``).  A member's result is what a
group of that member alone computes, bit for bit.

``RefineBatchHandle.curvature`` / ``hessian_product`` are the raw calls on a kept group handle; ``refine_estimate_batch(...,
curvature=k)`` runs the check on the handle that refined.  ``engine="python"`` is the dense ``eigh`` of
``curvature._python_curvature`` member by member; a member with fewer than 48 unknowns is answered that way whatever the engine.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import CURVATURE_BATCH, Cutter, ScoreCurvatureBatchInfo, bind, ptr, steps_and_converged
from .curvature import Curvature, _python_curvature
from .groups import chunks, grouped, paired, per_graph
from .marginals import _problem_and_point, _select
from .solver import _i32p, load_library
from .spectrum import MAX_MODES, MIN_DEVICE_UNKNOWNS, _layout
from .spectrum_batch import BASIS, BLOCK

# the symbols include/score_curvature_batch.h declares
CURVATURE_BATCH_SYMBOLS = list(CURVATURE_BATCH)


def _bind(lib: C.CDLL) -> C.CDLL:
    return bind(lib, CURVATURE_BATCH)


def batch_curvature(handle, points, k, rel_tol=1e-9, max_iters=200, shift=1e-8):
    """``score_refine_batch_curvature`` as it is, on a ``RefineBatchHandle``: ``points`` in the problems' own form.  Returns
    (return code, per member ``(values (k), vectors (k x n_g), residuals (k), v'(J'J)v (k), iterations, converged, h_max,
    c_max)``, the call's info record)."""
    probs = handle.probs
    _, poses, lms = handle._flat_points(points)
    lib = _bind(handle.lib)
    G, kk = len(probs), max(0, min(int(k), MAX_MODES))
    sizes = [int(prob.n) for prob in probs]
    values = np.full(max(1, G * kk), np.nan)
    vectors = np.full(max(1, kk * sum(sizes)), np.nan)
    res = np.full(max(1, G * kk), np.nan)
    gn = np.full(max(1, G * kk), np.nan)
    its = np.zeros(G, dtype=np.int32)
    h_max = np.full(G, np.nan)
    c_max = np.full(G, np.nan)
    info = ScoreCurvatureBatchInfo()
    rc = lib.score_refine_batch_curvature(handle.h, ptr(poses), ptr(lms), int(k), float(rel_tol), int(max_iters), float(shift),
                                          ptr(values), ptr(vectors), ptr(res), ptr(gn), ptr(its, _i32p), ptr(h_max), ptr(c_max),
                                          C.byref(info))
    if rc < 0:
        raise RuntimeError(f"score_refine_batch_curvature failed: {lib.score_last_error().decode()}")
    iterations, converged = steps_and_converged(its)
    cut, out = Cutter(), []
    for g, n in enumerate(sizes):
        out.append((cut(values, kk), cut(vectors, kk * n, (kk, n)), cut(res, kk), cut(gn, kk), int(iterations[g]), bool(converged[g]),
                    float(h_max[g]), float(c_max[g])))
    return rc, out, info.as_dict()


def batch_hessian_product(handle, points, V_per_member, exact=True):
    """``score_refine_batch_hessian_product`` as it is, on a ``RefineBatchHandle``: per member A_g V_g with A = E (``exact``)
    or J'J at ``points``.  ``V_per_member``: one n_g x c array per member (or a vector each), the same c in 1..16 for all.
    Returns the products in the shapes of the inputs."""
    probs = handle.probs
    if len(V_per_member) != len(probs):
        raise ValueError("one block of vectors per member expected")
    _, poses, lms = handle._flat_points(points)
    lib = _bind(handle.lib)
    shapes, blocks = [], []
    for g, (prob, V) in enumerate(zip(probs, V_per_member)):
        V = np.asarray(V, dtype=np.float64)
        cols = V.reshape(prob.n, -1) if V.ndim == 1 else V
        if cols.ndim != 2 or cols.shape[0] != prob.n:
            raise ValueError(f"member {g}: V must have {prob.n} rows")
        shapes.append(V.shape)
        blocks.append(np.ascontiguousarray(cols.T))
    n_cols = blocks[0].shape[0]
    if any(b.shape[0] != n_cols for b in blocks):
        raise ValueError("every member's V must have the same number of columns")
    flat = np.ascontiguousarray(np.concatenate([b.ravel() for b in blocks]))
    out = np.full(max(1, flat.size), np.nan)
    rc = lib.score_refine_batch_hessian_product(handle.h, ptr(poses), ptr(lms), 1 if exact else 0, ptr(flat), int(n_cols), ptr(out))
    if rc != 0:
        raise RuntimeError(f"score_refine_batch_hessian_product failed: {lib.score_last_error().decode()}")
    cut = Cutter()
    return [np.ascontiguousarray(cut(out, n_cols * prob.n, (n_cols, prob.n)).T).reshape(shape) for prob, shape in zip(probs, shapes)]


def indefinite_ritz(GA, GB, lib_path: Optional[str] = None):
    """``score_curvature_ritz``: ``spectrum_batch.device_ritz`` with the indefinite rule -- the lowest Ritz value may be
    negative.  Returns (theta (count x 16), coef (count x 48 x 16), status (count), kept (count)); theta and coef of a pencil
    that broke down are NaN."""
    lib = _bind(load_library(lib_path))
    GA = np.ascontiguousarray(GA, dtype=np.float64)
    GB = np.ascontiguousarray(GB, dtype=np.float64)
    if GA.ndim != 3 or GA.shape[1:] != (BASIS, BASIS) or GB.shape != GA.shape:
        raise ValueError(f"pencils of {BASIS} x {BASIS} expected, count of them in both arrays")
    count = GA.shape[0]
    theta = np.full((count, BLOCK), np.nan)
    coef = np.full((count, BASIS, BLOCK), np.nan)
    status = np.full(count, -1, dtype=np.int32)
    kept = np.full(count, -1, dtype=np.int32)
    rc = lib.score_curvature_ritz(count, ptr(GA), ptr(GB), ptr(theta), ptr(coef), ptr(status, _i32p), ptr(kept, _i32p))
    if rc != 0:
        raise RuntimeError(f"score_curvature_ritz failed: {lib.score_last_error().decode()}")
    return theta, coef, status, kept


def _curvature_of(prob, values, V, res, gn, h_max, rel_tol):
    names, first, size = _layout(prob)
    try:
        default_variables = _select(prob, None)[0]
    except ValueError:  # (a graph without landmarks whose only chain is the fixed pose)
        default_variables = []
    return Curvature(values, V, res, gn, names, first, size, h_max, rel_tol, default_variables)


def _host_member(prob, point, k, rel_tol, shift):
    values, V, res, gn, h_max, c_max = _python_curvature(prob, point, k)
    info = {"h_max": float(h_max), "shift": float(shift * h_max), "c_max": float(c_max), "iterations": 0, "unconverged": 0,
            "setup_ms": 0.0, "solve_ms": 0.0, "engine": "python"}
    return _curvature_of(prob, values, V, res, gn, h_max, rel_tol), info


def group_curvature(handle, probs, points, idx, k, rel_tol, max_iters, shift, who="hessian_spectrum_batch"):
    """One ``RefineBatchHandle.curvature`` call: ``[(Curvature, info), ...]`` member by member and the call's rounds.  A
    member with a pair that is not converged raises the single call's RuntimeError with its graph's index from ``idx``."""
    _, per, rec = handle.curvature(points, k, rel_tol, int(max_iters), shift)
    out = []
    for i, prob, (values, Vt, res, gn, its, converged, h_max, c_max) in zip(idx, probs, per):
        if not converged:
            bad = [j for j in range(k) if not res[j] <= rel_tol * h_max]
            what = ", ".join(f"mode {j} (residual {res[j]:.3e})" for j in bad) if bad else "the iteration broke down and"
            raise RuntimeError(f"{who}: graph {i}: {what} did not reach {rel_tol:g} * h_max = {rel_tol * h_max:.3e} in "
                               f"{max_iters} iterations")
        info = {"h_max": h_max, "shift": float(shift) * h_max, "c_max": c_max, "iterations": int(its), "unconverged": 0,
                "setup_ms": float(rec["setup_ms"]), "solve_ms": float(rec["solve_ms"]), "engine": "device"}
        out.append((_curvature_of(prob, values, np.ascontiguousarray(Vt.T), res, gn, h_max, rel_tol), info))
    return out, int(rec["rounds"])


def follow_up_curvature(handle, number, idx, probs, points, k, lib_path=None, solver_settings=None, rel_tol=1e-9, max_iters=200,
                        shift=1e-8):
    """``refine_estimate_batch(..., curvature=k)``: ``(Curvature, info)`` per member of a group at ``points``, on the group's
    own ``handle`` (None: the dense path).  A member below ``MIN_DEVICE_UNKNOWNS`` is answered by the dense path; the raw call
    takes every member of its handle, so the others of such a group then run on a handle of their own."""
    from .refine_batch import RefineBatchHandle

    out: list = [None] * len(idx)
    big = [g for g, prob in enumerate(probs) if handle is not None and prob.n >= MIN_DEVICE_UNKNOWNS]
    for g, prob in enumerate(probs):
        if g not in big:
            out[g] = _host_member(prob, points[g], k, rel_tol, shift)
    rounds = 0
    if big:
        sub = ([idx[g] for g in big], [probs[g] for g in big], [points[g] for g in big])
        if len(big) == len(probs):
            got, rounds = group_curvature(handle, sub[1], sub[2], sub[0], k, rel_tol, max_iters, shift, "refine_estimate_batch")
        else:
            with RefineBatchHandle(sub[1], lib_path, solver_settings) as own:
                got, rounds = group_curvature(own, sub[1], sub[2], sub[0], k, rel_tol, max_iters, shift, "refine_estimate_batch")
        for g, entry in zip(big, got):
            out[g] = entry
    for entry in out:
        entry[1]["group"], entry[1]["rounds"] = number, rounds
    return out


def _check_arguments(k, rel_tol, max_iters, shift):
    if int(k) != k or not 1 <= int(k) <= MAX_MODES:
        raise ValueError(f"k must be an integer in 1..{MAX_MODES}")
    if not rel_tol > 0 or not np.isfinite(rel_tol):
        raise ValueError("rel_tol must be positive")
    if int(max_iters) != max_iters or max_iters < 1:
        raise ValueError("max_iters must be at least 1")
    if not shift > 0 or not np.isfinite(shift):
        raise ValueError("shift must be positive")


def hessian_spectrum_batch(datas, results, k: int = 8, range_weights=None, loop_closure_weights=None, rel_tol: float = 1e-9,
                           max_iters: int = 200, shift: float = 1e-8, engine: str = "device", max_group: int = 64,
                           lib_path: Optional[str] = None, solver_settings: Optional[dict] = None):
    """``hessian_spectrum`` for many graphs at once: ``datas`` and ``results`` graph by graph, ``range_weights`` /
    ``loop_closure_weights`` None or lists with one entry per graph.  The graphs are grouped by dimension, in chunks of at
    most ``max_group`` (the rule of ``score_amd/groups.py``); each group is one device handle and one
    ``score_refine_batch_curvature`` call (``engine="device"``) or the dense ``eigh`` graph by graph (``engine="python"``).
    A graph with fewer than 48 unknowns is answered on the host by the dense path and says so in ``info["engine"]``.
    Returns a list of ``(Curvature, info)`` in input order: per graph what ``hessian_spectrum`` returns, plus ``group`` (the
    group's number) and ``rounds`` (lock-step rounds of the group's call; ``setup_ms`` and ``solve_ms`` are the group's).
    The single call's ValueErrors are raised with ``graph i:`` in front; a graph with a pair that is not converged raises the
    single call's RuntimeError with the graph's index."""
    from .refine_batch import RefineBatchHandle

    if engine not in ("device", "python"):
        raise ValueError("engine must be 'device' or 'python'")
    _check_arguments(k, rel_tol, max_iters, shift)
    datas, results = paired(datas, results, max_group)
    k = int(k)
    rws = per_graph(range_weights, len(datas), "range_weights")
    lws = per_graph(loop_closure_weights, len(datas), "loop_closure_weights")

    def member(i, data, res):
        prob, point = _problem_and_point(data, res, rws[i], lws[i])
        if k > prob.n:
            raise ValueError(f"k = {k} modes of a graph with {prob.n} unknowns")
        return prob, point

    out: list = [None] * len(datas)
    # (the placement is this call's own: a member below MIN_DEVICE_UNKNOWNS is answered on the host, the handle holds the rest)
    for number, chunk in chunks(grouped(datas, results, member), max_group):
        rounds = 0
        on_device = [m for m in chunk if engine == "device" and m[1].n >= MIN_DEVICE_UNKNOWNS]
        for i, prob, point in chunk:
            if engine == "python" or prob.n < MIN_DEVICE_UNKNOWNS:
                out[i] = _host_member(prob, point, k, rel_tol, shift)
        if on_device:
            idx, probs, points = [m[0] for m in on_device], [m[1] for m in on_device], [m[2] for m in on_device]
            with RefineBatchHandle(probs, lib_path, solver_settings) as h:
                got, rounds = group_curvature(h, probs, points, idx, k, rel_tol, max_iters, shift)
            for i, entry in zip(idx, got):
                out[i] = entry
        for i, _, _ in chunk:
            out[i][1]["group"], out[i][1]["rounds"] = number, rounds
    return out


__all__ = ["hessian_spectrum_batch", "batch_curvature", "batch_hessian_product", "indefinite_ritz", "group_curvature", "follow_up_curvature",
           "CURVATURE_BATCH_SYMBOLS", "ScoreCurvatureBatchInfo"]

"""The weakest modes of many refined estimates at once (include/score_spectrum_batch.h, csrc/score_spectrum_batch.hpp).

``information_spectrum`` takes one graph, builds one refinement handle and reads a 48 x 48 pencil back to the host in every
LOBPCG iteration.  ``information_spectrum_batch`` hands the graphs to the device as groups, by the rule of
``score_amd/groups.py``: the group handle's union matrix H = J'J is block diagonal, so one union vector carries
one vector of every member, and six blocks of 16 union vectors run the block eigensolver on every member in lock-step
rounds (``score_refine_batch_spectrum``).  The Rayleigh-Ritz step runs on the device, one workgroup per member.  Every
member has its own shift, tolerance, done words, mode and verdict: a member's result is what a group of that member alone
computes, bit for bit.

``RefineBatchHandle.spectrum`` is the raw call on a kept group handle, so a study refines, takes covariances and looks for
undetermined landmarks with one create.  ``engine="python"`` is the dense ``eigh`` of ``spectrum._python_spectrum`` member
by member; a member with fewer than 48 unknowns is answered that way whatever the engine.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from .bindings import SPECTRUM_BATCH, Cutter, ScoreSpectrumBatchInfo, bind, ptr, steps_and_converged
from .groups import chunks, grouped, paired, per_graph
from .marginals import _problem_and_point, _select
from .solver import _i32p, load_library
from .spectrum import MAX_MODES, MIN_DEVICE_UNKNOWNS, Modes, _layout, _python_spectrum

# the symbols include/score_spectrum_batch.h declares
SPECTRUM_BATCH_SYMBOLS = list(SPECTRUM_BATCH)
BLOCK = 16            # vectors iterated per member
BASIS = 3 * BLOCK     # columns of [X | W | P]: the order of a pencil
RITZ_OK, RITZ_NO_P, RITZ_BREAKDOWN = 0, 1, 2


def _bind(lib: C.CDLL) -> C.CDLL:
    return bind(lib, SPECTRUM_BATCH)


def batch_spectrum(handle, points, k, rel_tol=1e-9, max_iters=200, shift=1e-8):
    """``score_refine_batch_spectrum`` as it is, on a ``RefineBatchHandle``: ``points`` in the problems' own form.  Returns
    (return code, per member ``(values (k), vectors (k x n_g), residuals (k), iterations, converged, h_max)``, the call's info
    record)."""
    probs = handle.probs
    _, poses, lms = handle._flat_points(points)
    lib = _bind(handle.lib)
    G, kk = len(probs), max(0, min(int(k), MAX_MODES))
    sizes = [int(prob.n) for prob in probs]
    values = np.full(max(1, G * kk), np.nan)
    vectors = np.full(max(1, kk * sum(sizes)), np.nan)
    res = np.full(max(1, G * kk), np.nan)
    its = np.zeros(G, dtype=np.int32)
    h_max = np.full(G, np.nan)
    info = ScoreSpectrumBatchInfo()
    rc = lib.score_refine_batch_spectrum(handle.h, ptr(poses), ptr(lms), int(k), float(rel_tol), int(max_iters), float(shift),
                                         ptr(values), ptr(vectors), ptr(res), ptr(its, _i32p), ptr(h_max), C.byref(info))
    if rc < 0:
        raise RuntimeError(f"score_refine_batch_spectrum failed: {lib.score_last_error().decode()}")
    iterations, converged = steps_and_converged(its)
    cut, out = Cutter(), []
    for g, n in enumerate(sizes):
        out.append((cut(values, kk), cut(vectors, kk * n, (kk, n)), cut(res, kk), int(iterations[g]), bool(converged[g]), float(h_max[g])))
    return rc, out, info.as_dict()


def device_ritz(GA, GB, lib_path: Optional[str] = None):
    """``score_spectrum_ritz``: the device Rayleigh-Ritz step alone on ``count`` pencils (GA, GB: count x 48 x 48).  Returns
    (theta (count x 16), coef (count x 48 x 16), status (count), kept (count)); theta and coef of a pencil that broke down
    are NaN."""
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
    rc = lib.score_spectrum_ritz(count, ptr(GA), ptr(GB), ptr(theta), ptr(coef), ptr(status, _i32p), ptr(kept, _i32p))
    if rc != 0:
        raise RuntimeError(f"score_spectrum_ritz failed: {lib.score_last_error().decode()}")
    return theta, coef, status, kept


def _modes_of(prob, values, V, res, h_max, rel_tol):
    names, first, size = _layout(prob)
    try:
        default_variables = _select(prob, None)[0]
    except ValueError:  # (a graph without landmarks whose only chain is the fixed pose)
        default_variables = []
    return Modes(values, V, res, names, first, size, h_max, rel_tol, default_variables)


def _host_member(prob, point, k, rel_tol, shift):
    values, V, res, h_max = _python_spectrum(prob, point, k)
    info = {"h_max": float(h_max), "shift": float(shift * h_max), "iterations": 0, "unconverged": 0, "setup_ms": 0.0, "solve_ms": 0.0,
            "engine": "python"}
    return _modes_of(prob, values, V, res, h_max, rel_tol), info


def information_spectrum_batch(datas, results, k: int = 8, range_weights=None, loop_closure_weights=None, rel_tol: float = 1e-9,
                               max_iters: int = 200, shift: float = 1e-8, engine: str = "device", max_group: int = 64,
                               lib_path: Optional[str] = None, solver_settings: Optional[dict] = None):
    """``information_spectrum`` for many graphs at once: ``datas`` and ``results`` graph by graph, ``range_weights`` /
    ``loop_closure_weights`` None or lists with one entry per graph.  The graphs are grouped by dimension, in chunks of at
    most ``max_group`` (the rule of ``score_amd/groups.py``); each group is one device handle and one
    ``score_refine_batch_spectrum`` call (``engine="device"``) or the dense ``eigh`` graph by graph (``engine="python"``).
    A graph with fewer than 48 unknowns is answered on the host by the dense path and says so in ``info["engine"]``.
    Returns a list of ``(Modes, info)`` in input order: per graph what ``information_spectrum`` returns, plus ``group`` (the
    group's number) and ``rounds`` (lock-step rounds of the group's call; ``setup_ms`` and ``solve_ms`` are the group's).
    The single call's ValueErrors are raised with ``graph i:`` in front; a graph with a pair that is not converged raises the
    single call's RuntimeError with the graph's index."""
    from .refine_batch import RefineBatchHandle

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
            probs, points = [m[1] for m in on_device], [m[2] for m in on_device]
            with RefineBatchHandle(probs, lib_path, solver_settings) as h:
                _, per, rec = h.spectrum(points, k, rel_tol, int(max_iters), shift)
            rounds = int(rec["rounds"])
            for (i, prob, _), (values, Vt, res, its, converged, h_max) in zip(on_device, per):
                if not converged:
                    bad = [j for j in range(k) if not res[j] <= rel_tol * h_max]
                    what = ", ".join(f"mode {j} (residual {res[j]:.3e})" for j in bad) if bad else "the iteration broke down and"
                    raise RuntimeError(f"information_spectrum_batch: graph {i}: {what} did not reach {rel_tol:g} * h_max = "
                                       f"{rel_tol * h_max:.3e} in {max_iters} iterations")
                info = {"h_max": h_max, "shift": float(shift) * h_max, "iterations": int(its), "unconverged": 0,
                        "setup_ms": float(rec["setup_ms"]), "solve_ms": float(rec["solve_ms"]), "engine": "device"}
                out[i] = (_modes_of(prob, values, np.ascontiguousarray(Vt.T), res, h_max, rel_tol), info)
        for i, _, _ in chunk:
            out[i][1]["group"], out[i][1]["rounds"] = number, rounds
    return out


__all__ = ["information_spectrum_batch", "batch_spectrum", "device_ritz", "SPECTRUM_BATCH_SYMBOLS", "ScoreSpectrumBatchInfo"]
